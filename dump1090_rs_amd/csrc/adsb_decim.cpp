// adsb_decim.cpp -- the host side of the decimator (include/adsb_hip.h, "Decimation"): the handle and its argument
// checks, the count arithmetic (all of it on the host: no call synchronises to learn a count), the staging and the piece
// loop of adsb_decim_demod_iq, and the default taps.  The kernels are adsb_decim.hip's.  (The mixer's host side is
// adsb_mix.cpp's: this unit hands it its handle's mixer, and a launch the mixer's parameters.)
#include <cmath>

#include "adsb_ctx.h"

using namespace adsb::host;

// The filter's history -- the last n_taps - 1 inputs, widened -- lives on the device in two buffers that take turns, the
// way the carry of carry-over mode is handed on: a call reads `cur` and writes the other one.  `consumed` (P) is the
// host's.
struct adsb_decim {
    adsb_ctx *ctx = nullptr;
    uint32_t factor = 0, n_taps = 0, shift = 0;
    int32_t *d_taps = nullptr;               // padded with zeros to a multiple of eight
    uint32_t *d_hist[2] = {nullptr, nullptr};
    int cur = 0;
    uint64_t consumed = 0;
    // adsb_decim_demod_iq: one piece's inputs and outputs in device memory (allocated on first use)
    void *d_in = nullptr;
    size_t in_bytes = 0;
    void *d_out = nullptr;
    size_t out_bytes = 0;
    Mixer mix;
    float scale = kInDefaultScale;   // CF32: g of q(x) (adsb_fmt.cpp)
    InStat instat;                   // input statistics (adsb_instat.cpp): off unless asked for
    Registry mem;   // owns the five buffers above, the mixer's table and the statistics' accumulator
};

namespace adsb {
namespace host {
MixerOwner mixer_of(adsb_decim *d) { return {d->ctx, &d->mem, &d->mix}; }
float *scale_of(adsb_decim *d) { return &d->scale; }
InStatOwner instat_of(adsb_decim *d) { return {d->ctx, &d->mem, &d->instat, 1u}; }
}  // namespace host
}  // namespace adsb

namespace {

// outputs of a call of n_in inputs behind `consumed`: the n with consumed <= n D < consumed + n_in
inline uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }
inline uint64_t out_count(const adsb_decim *d, uint64_t n_in)
{
    return ceil_div(d->consumed + n_in, d->factor) - ceil_div(d->consumed, d->factor);
}
// ... and the input index, within the call, of the first of them
inline uint32_t first_output_at(const adsb_decim *d)
{
    return (uint32_t)((d->factor - d->consumed % d->factor) % d->factor);
}

// One call on the context's input stream: the kernels, the history's turn and P.  No wait.
int run_on_stream(adsb_decim *d, int format, const void *d_in, uint64_t n_in, void *d_out, uint64_t n_out)
{
    adsb_ctx *c = d->ctx;
    if (n_in == 0) return ADSB_OK;
    DecimParams p{};
    p.src = d_in;
    p.n_in = n_in;
    p.hist_prev = d->d_hist[d->cur];
    p.hist_next = d->d_hist[d->cur ^ 1];
    p.taps = d->d_taps;
    p.u8_table = format == ADSB_DECIM_8BIT ? c->d_u8_table : nullptr;
    p.format = (uint32_t)format;
    p.scale = d->scale;
    p.out = static_cast<uint32_t *>(d_out);
    p.n_out = n_out;
    p.factor = d->factor, p.n_taps = d->n_taps, p.shift = d->shift;
    p.first = first_output_at(d);
    p.row_len = decim_row_len(d->factor, d->n_taps);
    p.recip = ((1u << 20) + d->factor - 1u) / d->factor;
    p.mix = mixer_params(d->mix, d->consumed);
    // (the raw input counted first, on the same stream: a small call's input is still in cache for the filter)
    if (d->instat.on)
        if (int rc = d->instat.count(c, d->instat, format, d->scale, d_in, n_in)) return rc;
    if (int e = launch_decim(p, c->stream)) return fail(c, (hipError_t)e, "launch_decim");
    // (the next pass reads what this put on the context's own stream: order_behind_input)
    if (c->stream == c->own_stream) c->own_stream_dirty = true;
    if (d->n_taps > 1) d->cur ^= 1;
    d->consumed += n_in;
    return ADSB_OK;
}

int ensure_buffer(adsb_ctx *c, Registry &mem, void **buf, size_t *have, size_t bytes)
{
    if (bytes <= *have) return ADSB_OK;
    mem.release(buf);
    *have = 0;
    HIP_TRY(c, mem.add(Registry::kDevice, buf, bytes));
    *have = bytes;
    return ADSB_OK;
}

int demod_host(adsb_decim *d, int format, const void *host_iq, size_t n_in, adsb_msg *out, size_t cap, size_t *n_out)
{
    adsb_ctx *c = d->ctx;
    ADSB_ON_DEVICE(c);
    if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
    const size_t bps = in_bytes_per_sample((uint32_t)format);
    const char *in = static_cast<const char *>(host_iq);
    const uint64_t D = d->factor, total_out = out_count(d, n_in);
    // pieces of whole output buffers, at most what one pass of a small call takes
    const uint64_t piece_out = std::min<uint64_t>(c->max_chunks, kInlineTailChunks) * (uint64_t)kChunkSamples;
    std::vector<adsb_msg> msgs;
    adsb_stats total{};
    std::vector<adsb_signal_stats> sig;
    c->sig_out.clear();
    uint64_t in_done = 0;
    for (uint64_t out_done = 0; out_done < total_out;) {
        const uint64_t n_o = std::min(piece_out, total_out - out_done);
        // the inputs up to the one in front of the next piece's first output; the last piece takes what is left
        const uint64_t n_i = out_done + n_o == total_out ? n_in - in_done : first_output_at(d) + n_o * D;
        if (int rc = ensure_buffer(c, d->mem, &d->d_in, &d->in_bytes, std::min<uint64_t>(n_in, (piece_out + 1) * D) * bps)) return rc;
        if (int rc = ensure_buffer(c, d->mem, &d->d_out, &d->out_bytes, std::min(piece_out, total_out) * 4)) return rc;
        HIP_TRY(c, hipMemcpyAsync(d->d_in, in + in_done * bps, n_i * bps, hipMemcpyHostToDevice, c->stream));
        if (c->stream == c->own_stream) c->own_stream_dirty = true;
        if (int rc = run_on_stream(d, format, d->d_in, n_i, d->d_out, n_o)) return rc;
        std::vector<adsb_msg> part;
        if (int rc = demod_device(c, d->d_out, n_o, part)) return rc;
        append_piece(c, part, out_done, msgs, total, sig);
        in_done += n_i;
        out_done += n_o;
    }
    if (in_done < n_in) {
        // inputs that reach no output (only a call without any has them): they still enter the history
        const uint64_t n_i = n_in - in_done;
        if (int rc = ensure_buffer(c, d->mem, &d->d_in, &d->in_bytes, n_i * bps)) return rc;
        HIP_TRY(c, hipMemcpyAsync(d->d_in, in + in_done * bps, n_i * bps, hipMemcpyHostToDevice, c->stream));
        if (c->stream == c->own_stream) c->own_stream_dirty = true;
        if (int rc = run_on_stream(d, format, d->d_in, n_i, nullptr, 0)) return rc;
        // (the staging is reused by the next call: this one has nothing behind it that waits)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    total.n_samples = total_out;
    c->stats = total;
    c->sig_out.swap(sig);
    return deliver(c, msgs, out, cap, n_out);
}

}  // namespace

extern "C" {

int adsb_decim_create(adsb_ctx *c, uint32_t factor, const int16_t *taps, uint32_t n_taps, uint32_t shift, adsb_decim **out)
try {
    if (out) *out = nullptr;
    if (!c || !out || !taps) return ADSB_ERR_INVALID;
    if (factor < kDecimMinFactor || factor > kDecimMaxFactor || n_taps < 1 || n_taps > kDecimMaxTaps || shift > kDecimMaxShift)
        return ADSB_ERR_INVALID;
    uint32_t abs_sum = 0;   // (an int32 accumulator never wraps: 65534 * 32768 + 32768 < 2^31)
    for (uint32_t k = 0; k < n_taps; k++) abs_sum += (uint32_t)std::abs((int)taps[k]);
    if (abs_sum > 65534u) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(c);
    adsb_decim *d = new adsb_decim;
    d->ctx = c;
    d->factor = factor, d->n_taps = n_taps, d->shift = shift;
    std::vector<int32_t> padded((n_taps + 7u) & ~7u, 0);
    for (uint32_t k = 0; k < n_taps; k++) padded[k] = taps[k];
    hipError_t e = d->mem.add(Registry::kDevice, (void **)&d->d_taps, padded.size() * sizeof(int32_t));
    for (int b = 0; b < 2 && e == hipSuccess; b++) e = d->mem.add(Registry::kDevice, (void **)&d->d_hist[b], kDecimHistWords * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d->d_taps, padded.data(), padded.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    for (int b = 0; b < 2 && e == hipSuccess; b++) e = hipMemset(d->d_hist[b], 0, kDecimHistWords * sizeof(uint32_t));
    if (e != hipSuccess) {
        const int rc = e == hipErrorOutOfMemory ? ADSB_ERR_NOMEM : fail(c, e, "adsb_decim_create");
        adsb_decim_destroy(d);
        return rc;
    }
    *out = d;
    return ADSB_OK;
} ADSB_ABI_CATCH

void adsb_decim_destroy(adsb_decim *d)
{
    if (!d) return;
    {
        DeviceGuard guard(d->ctx->device);
        // (what the handle put on the stream may still read its buffers)
        (void)hipStreamSynchronize(d->ctx->stream);
        d->mem.release_all();
    }
    delete d;
}

int adsb_decim_reset(adsb_decim *d)
try {
    if (!d) return ADSB_ERR_INVALID;
    adsb_ctx *c = d->ctx;
    ADSB_ON_DEVICE(c);
    HIP_TRY(c, hipMemsetAsync(d->d_hist[d->cur], 0, kDecimHistWords * sizeof(uint32_t), c->stream));
    d->consumed = 0;
    return ADSB_OK;
} ADSB_ABI_CATCH

uint32_t adsb_mix_get_decim(const adsb_decim *d) { return d ? d->mix.period : 0; }
float adsb_fmt_get_scale_decim(const adsb_decim *d) { return d ? d->scale : 0.0f; }

int adsb_decim_out_count(const adsb_decim *d, size_t n_in, size_t *n_out)
{
    if (!d || !n_out) return ADSB_ERR_INVALID;
    *n_out = (size_t)out_count(d, n_in);
    return ADSB_OK;
}

int adsb_decim_run_device(adsb_decim *d, int format, const void *device_in, size_t n_in, void *device_out_cs16, size_t out_cap,
                          size_t *n_out)
try {
    if (!d || !n_out || !format_ok(format) || (!device_in && n_in)) return ADSB_ERR_INVALID;
    if (((uintptr_t)device_in & 15u) != 0 || ((uintptr_t)device_out_cs16 & 15u) != 0) return ADSB_ERR_INVALID;
    const uint64_t n = out_count(d, n_in);
    *n_out = (size_t)n;
    if (n > out_cap) return ADSB_ERR_CAPACITY;   // nothing consumed
    if (n && !device_out_cs16) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(d->ctx);
    return run_on_stream(d, format, device_in, n_in, device_out_cs16, n);
} ADSB_ABI_CATCH

int adsb_decim_demod_iq(adsb_decim *d, int format, const void *host_iq, size_t n_in, adsb_msg *out, size_t cap, size_t *n_out)
try {
    if (!d || !format_ok(format) || (!host_iq && n_in) || (!out && cap)) return ADSB_ERR_INVALID;
    return demod_host(d, format, host_iq, n_in, out, cap, n_out);
} ADSB_ABI_CATCH

int adsb_decim_default_taps(uint32_t factor, int16_t *taps, size_t cap, uint32_t *n_taps, uint32_t *shift)
try {
    if (factor < kDecimMinFactor || factor > kDecimMaxFactor || !n_taps || (!taps && cap)) return ADSB_ERR_INVALID;
    const uint32_t n = 8 * factor + 1;
    *n_taps = n;
    if (shift) *shift = 15;
    if (cap < n) return ADSB_ERR_CAPACITY;
    // a sinc with its cutoff at 1.2 MHz of factor x 2.4 MS/s -- 1 / (2 factor) cycles per sample -- under a Hamming window
    const double pi = 3.14159265358979323846;
    const int half = 4 * (int)factor;
    std::vector<double> w(n);
    double sum = 0;
    for (int i = 0; i <= 2 * half; i++) {
        const double t = (double)(i - half) / (double)factor;   // 2 fc (i - centre)
        const double sinc = i == half ? 1.0 : std::sin(pi * t) / (pi * t);
        w[i] = sinc * (0.54 - 0.46 * std::cos(2.0 * pi * (double)i / (double)(2 * half)));
        sum += w[i];
    }
    // rounded from one half and mirrored, so that the symmetry does not hang on libm; the centre tap takes the rest
    long total = 0;
    for (int i = 0; i < half; i++) {
        const long v = std::lround(w[i] / sum * 32768.0);
        taps[i] = taps[2 * half - i] = (int16_t)v;
        total += 2 * v;
    }
    taps[half] = (int16_t)(32768 - total);
    return ADSB_OK;
} ADSB_ABI_CATCH

uint32_t adsb_decim_selftest_tile(void) { return kDecimTile; }

}  // extern "C"
