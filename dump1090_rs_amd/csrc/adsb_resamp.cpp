// adsb_resamp.cpp -- the host side of the rational resampler (include/adsb_hip.h, "Resampling"): the handle and its
// argument checks, the count arithmetic (all of it 64-bit arithmetic on the host: no call synchronises to learn a count),
// the staging and the piece loop of adsb_resamp_demod_iq, the default taps and the ratio of a sample rate.  The kernels
// are adsb_resamp.hip's.
#include <cmath>
#include <numeric>

#include "adsb_resamp_host.h"

using namespace adsb::host;

// The filter's history -- the last K - 1 inputs, widened -- lives on the device in two buffers that take turns, as the
// decimator's does: a call reads `cur` and writes the other one.  `consumed` (P) is the host's.
struct adsb_resamp {
    adsb_ctx *ctx = nullptr;
    uint32_t up = 0, down = 0, n_taps = 0, k_taps = 0, k_pad = 0, shift = 0;
    int32_t *d_taps = nullptr;               // polyphase order, every phase padded with zeros to k_pad
    uint32_t *d_hist[2] = {nullptr, nullptr};
    int cur = 0;
    uint64_t consumed = 0;
    // adsb_resamp_demod_iq: one piece's inputs and outputs in device memory (allocated on first use)
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
MixerOwner mixer_of(adsb_resamp *r) { return {r->ctx, &r->mem, &r->mix}; }
float *scale_of(adsb_resamp *r) { return &r->scale; }
InStatOwner instat_of(adsb_resamp *r) { return {r->ctx, &r->mem, &r->instat, 1u}; }
}  // namespace host
}  // namespace adsb

namespace {

// (the count arithmetic is adsb_resamp_host.h's, shared with the banks)
inline uint64_t out_count(const adsb_resamp *r, uint64_t n_in) { return adsb::host::out_count(r->up, r->down, r->consumed, n_in); }
inline uint64_t inputs_for(const adsb_resamp *r, uint64_t need) { return adsb::host::inputs_for(r->up, r->down, r->consumed, need); }

// One call on the context's input stream: the kernels, the history's turn and P.  No wait.
int run_on_stream(adsb_resamp *r, int format, const void *d_in, uint64_t n_in, void *d_out, uint64_t n_out)
{
    adsb_ctx *c = r->ctx;
    if (n_in == 0) return ADSB_OK;
    const uint32_t L = r->up, M = r->down;
    ResampParams p{};
    p.src = d_in;
    p.n_in = n_in;
    p.hist_prev = r->d_hist[r->cur];
    p.hist_next = r->d_hist[r->cur ^ 1];
    p.u8_table = format == ADSB_DECIM_8BIT ? c->d_u8_table : nullptr;
    p.format = (uint32_t)format;
    p.scale = r->scale;
    p.out = static_cast<uint32_t *>(d_out);
    p.n_out = n_out;
    filter_params(p, L, M, r->k_taps, r->k_pad, r->shift, r->d_taps);
    first_output(L, M, r->consumed, &p.p0, &p.q0);
    p.mix = mixer_params(r->mix, r->consumed);
    // (the raw input counted first, on the same stream: a small call's input is still in cache for the filter)
    if (r->instat.on)
        if (int rc = r->instat.count(c, r->instat, format, r->scale, d_in, n_in)) return rc;
    if (int e = launch_resamp(p, c->stream)) return fail(c, (hipError_t)e, "launch_resamp");
    // (the next pass reads what this put on the context's own stream: order_behind_input)
    if (c->stream == c->own_stream) c->own_stream_dirty = true;
    if (r->k_taps > 1) r->cur ^= 1;
    r->consumed += n_in;
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

int copy_in_and_run(adsb_resamp *r, int format, const char *in, uint64_t n_i, size_t bps, void *d_out, uint64_t n_o)
{
    adsb_ctx *c = r->ctx;
    if (n_i == 0) return ADSB_OK;
    if (int rc = ensure_buffer(c, r->mem, &r->d_in, &r->in_bytes, n_i * bps)) return rc;
    HIP_TRY(c, hipMemcpyAsync(r->d_in, in, n_i * bps, hipMemcpyHostToDevice, c->stream));
    if (c->stream == c->own_stream) c->own_stream_dirty = true;
    return run_on_stream(r, format, r->d_in, n_i, d_out, n_o);
}

int demod_host(adsb_resamp *r, int format, const void *host_iq, size_t n_in, adsb_msg *out, size_t cap, size_t *n_out)
{
    adsb_ctx *c = r->ctx;
    ADSB_ON_DEVICE(c);
    if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
    const size_t bps = in_bytes_per_sample((uint32_t)format);
    const char *in = static_cast<const char *>(host_iq);
    const uint64_t total_out = out_count(r, n_in);
    // pieces of whole output buffers, at most what one pass of a small call takes
    const uint64_t piece_out = std::min<uint64_t>(c->max_chunks, kInlineTailChunks) * (uint64_t)kChunkSamples;
    std::vector<adsb_msg> msgs;
    adsb_stats total{};
    std::vector<adsb_signal_stats> sig;
    c->sig_out.clear();
    // the staged outputs: a piece's, in front of them the output the piece before produced beyond its last buffer, and
    // room for this piece's own.  (Where L > M two consecutive outputs can share their newest input, and an output-buffer
    // boundary can fall between them: then no cut of the input produces a whole number of buffers.)
    if (total_out)
        if (int rc = ensure_buffer(c, r->mem, &r->d_out, &r->out_bytes, (std::min(piece_out, total_out) + 2) * 4)) return rc;
    // ... and the staged inputs, sized once for the longest piece: the inputs from behind P up to the newest input of
    // piece_out + 1 outputs on, and (the last piece) the inputs behind that which reach no output
    if (n_in) {
        const uint64_t most = std::min<uint64_t>(n_in, (piece_out + 2) * (uint64_t)r->down / r->up + 3);
        if (int rc = ensure_buffer(c, r->mem, &r->d_in, &r->in_bytes, most * bps)) return rc;
    }
    uint32_t *staged = static_cast<uint32_t *>(r->d_out);
    uint64_t in_done = 0, carried = 0;   // carried: 0 or 1 (L <= 2 M)
    for (uint64_t out_done = 0; out_done < total_out;) {
        const uint64_t n_o = std::min(piece_out, total_out - out_done), need = n_o - carried;
        const bool last = out_done + n_o == total_out;
        // the inputs up to the newest one of the piece's last output; the last piece takes what is left
        const uint64_t n_i = last ? n_in - in_done : need ? inputs_for(r, need) : 0;
        const uint64_t made = out_count(r, n_i);   // need, or one more
        if (int rc = copy_in_and_run(r, format, in + in_done * bps, n_i, bps, staged + carried, made)) return rc;
        std::vector<adsb_msg> part;
        if (int rc = demod_device(c, staged, n_o, part)) return rc;
        append_piece(c, part, out_done, msgs, total, sig);
        carried = carried + made - n_o;
        if (carried) {
            HIP_TRY(c, hipMemcpyAsync(staged, staged + n_o, carried * 4, hipMemcpyDeviceToDevice, c->stream));
            if (c->stream == c->own_stream) c->own_stream_dirty = true;
        }
        in_done += n_i;
        out_done += n_o;
    }
    if (in_done < n_in) {
        // inputs that reach no output (only a call without any has them): they still enter the history
        if (int rc = copy_in_and_run(r, format, in + in_done * bps, n_in - in_done, bps, nullptr, 0)) return rc;
    }
    // (the staging is reused by the next call: this one leaves nothing behind it that reads or writes it)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    total.n_samples = total_out;
    c->stats = total;
    c->sig_out.swap(sig);
    return deliver(c, msgs, out, cap, n_out);
}

}  // namespace

extern "C" {

int adsb_resamp_create(adsb_ctx *c, uint32_t up, uint32_t down, const int16_t *taps, uint32_t n_taps, uint32_t shift,
                       adsb_resamp **out)
try {
    if (out) *out = nullptr;
    if (!c || !out || !taps) return ADSB_ERR_INVALID;
    uint32_t k_taps = 0;
    if (!filter_ok(up, down, taps, n_taps, shift, &k_taps)) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(c);
    adsb_resamp *r = new adsb_resamp;
    r->ctx = c;
    r->up = up, r->down = down, r->n_taps = n_taps, r->k_taps = k_taps, r->k_pad = (k_taps + 7u) & ~7u, r->shift = shift;
    const std::vector<int32_t> pp = polyphase(taps, n_taps, up, r->k_pad);
    hipError_t e = r->mem.add(Registry::kDevice, (void **)&r->d_taps, pp.size() * sizeof(int32_t));
    for (int b = 0; b < 2 && e == hipSuccess; b++) e = r->mem.add(Registry::kDevice, (void **)&r->d_hist[b], kResampHistWords * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(r->d_taps, pp.data(), pp.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    for (int b = 0; b < 2 && e == hipSuccess; b++) e = hipMemset(r->d_hist[b], 0, kResampHistWords * sizeof(uint32_t));
    if (e != hipSuccess) {
        const int rc = e == hipErrorOutOfMemory ? ADSB_ERR_NOMEM : fail(c, e, "adsb_resamp_create");
        adsb_resamp_destroy(r);
        return rc;
    }
    *out = r;
    return ADSB_OK;
} ADSB_ABI_CATCH

void adsb_resamp_destroy(adsb_resamp *r)
{
    if (!r) return;
    {
        DeviceGuard guard(r->ctx->device);
        // (what the handle put on the stream may still read its buffers)
        (void)hipStreamSynchronize(r->ctx->stream);
        r->mem.release_all();
    }
    delete r;
}

int adsb_resamp_reset(adsb_resamp *r)
try {
    if (!r) return ADSB_ERR_INVALID;
    adsb_ctx *c = r->ctx;
    ADSB_ON_DEVICE(c);
    HIP_TRY(c, hipMemsetAsync(r->d_hist[r->cur], 0, kResampHistWords * sizeof(uint32_t), c->stream));
    r->consumed = 0;
    return ADSB_OK;
} ADSB_ABI_CATCH

uint32_t adsb_mix_get_resamp(const adsb_resamp *r) { return r ? r->mix.period : 0; }
float adsb_fmt_get_scale_resamp(const adsb_resamp *r) { return r ? r->scale : 0.0f; }

int adsb_resamp_out_count(const adsb_resamp *r, size_t n_in, size_t *n_out)
{
    if (!r || !n_out) return ADSB_ERR_INVALID;
    *n_out = (size_t)out_count(r, n_in);
    return ADSB_OK;
}

int adsb_resamp_run_device(adsb_resamp *r, int format, const void *device_in, size_t n_in, void *device_out_cs16, size_t out_cap,
                           size_t *n_out)
try {
    if (!r || !n_out || !format_ok(format) || (!device_in && n_in)) return ADSB_ERR_INVALID;
    if (((uintptr_t)device_in & 15u) != 0 || ((uintptr_t)device_out_cs16 & 15u) != 0) return ADSB_ERR_INVALID;
    const uint64_t n = out_count(r, n_in);
    *n_out = (size_t)n;
    if (n > out_cap) return ADSB_ERR_CAPACITY;   // nothing consumed
    if (n && !device_out_cs16) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(r->ctx);
    return run_on_stream(r, format, device_in, n_in, device_out_cs16, n);
} ADSB_ABI_CATCH

int adsb_resamp_demod_iq(adsb_resamp *r, int format, const void *host_iq, size_t n_in, adsb_msg *out, size_t cap, size_t *n_out)
try {
    if (!r || !format_ok(format) || (!host_iq && n_in) || (!out && cap)) return ADSB_ERR_INVALID;
    return demod_host(r, format, host_iq, n_in, out, cap, n_out);
} ADSB_ABI_CATCH

int adsb_resamp_default_taps(uint32_t up, uint32_t down, int16_t *taps, size_t cap, uint32_t *n_taps, uint32_t *shift)
try {
    if (!ratio_ok(up, down) || !n_taps || (!taps && cap)) return ADSB_ERR_INVALID;
    const uint32_t big = std::max(up, down), n = 8 * big + 1;
    *n_taps = n;
    if (shift) *shift = 14;
    if (cap < n) return ADSB_ERR_CAPACITY;
    // a sinc over the zero-stuffed rate with its cutoff at half the lower of the two rates -- 1 / (2 max(L, M)) cycles per
    // sample -- under a Hamming window, scaled to sum L 2^14: every phase sums to about 2^14
    const double pi = 3.14159265358979323846;
    const int half = 4 * (int)big;
    std::vector<double> w(n);
    double sum = 0;
    for (int i = 0; i <= 2 * half; i++) {
        const double t = (double)(i - half) / (double)big;   // 2 fc (i - centre)
        const double sinc = i == half ? 1.0 : std::sin(pi * t) / (pi * t);
        w[i] = sinc * (0.54 - 0.46 * std::cos(2.0 * pi * (double)i / (double)(2 * half)));
        sum += w[i];
    }
    // rounded from one half and mirrored, so that the symmetry does not hang on libm
    const double scale = (double)up * 16384.0 / sum;
    for (int i = 0; i <= half; i++) {
        const long v = std::lround(w[i] * scale);
        if (v < -32768 || v > 32767) return ADSB_ERR_INVALID;
        taps[i] = taps[2 * half - i] = (int16_t)v;
    }
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_resamp_ratio_for_rate(uint32_t rate_hz, uint32_t *up, uint32_t *down)
{
    if (!up || !down || !rate_hz) return ADSB_ERR_INVALID;
    const uint32_t g = std::gcd(2400000u, rate_hz);
    *up = 2400000u / g, *down = rate_hz / g;
    return ratio_ok(*up, *down) ? ADSB_OK : ADSB_ERR_INVALID;
}

int adsb_resamp_plan(uint32_t up, uint32_t down, uint64_t consumed, uint64_t n_in, uint64_t *first_n, uint64_t *n_out)
{
    // (consumed + n_in and the counts themselves stay within 64 bits: streams of less than 2^56 inputs)
    if (!ratio_ok(up, down) || !first_n || !n_out || consumed >> 56 || n_in >> 56) return ADSB_ERR_INVALID;
    plan(up, down, consumed, n_in, first_n, n_out);
    return ADSB_OK;
}

uint32_t adsb_resamp_selftest_tile(uint32_t up, uint32_t down) { return ratio_ok(up, down) ? up * resamp_rows(up, down) : 0; }

}  // extern "C"
