// adsb_bank.cpp -- the host side of a resampler bank (include/adsb_hip.h, "Resampler banks"): N streams of one ratio and
// one filter, each with its own P and its own history, advanced by one call and one k_resamp_bank launch.  Per stream the
// arithmetic is the single resampler's (adsb_resamp_host.h); the kernels are adsb_resamp.hip's.  What a call's runs have
// of their own travels to the device as descriptors, through a fixed number of blocks used in rotation: a block is filled
// in pinned memory, copied on the stream in front of the launch that reads it, and guarded by an event recorded behind
// that launch -- no call waits unless kBankBlocks calls are still in flight behind it.
#include "adsb_resamp_host.h"

using namespace adsb::host;

namespace {
constexpr uint32_t kBankBlocks = 4;
}

struct adsb_bank {
    adsb_ctx *ctx = nullptr;
    uint32_t n_streams = 0, up = 0, down = 0, n_taps = 0, k_taps = 0, k_pad = 0, shift = 0;
    int32_t *d_taps = nullptr;                  // polyphase order, every phase padded with zeros to k_pad
    uint32_t *d_hist[2] = {nullptr, nullptr};   // n_streams x kResampHistWords each: stream i's two buffers take turns
    std::vector<uint8_t> cur;                   // per stream: which of the two the next call reads
    std::vector<uint64_t> consumed;             // per stream: P
    std::vector<uint32_t> named;                // per stream: the last call that named it (a stream named twice)
    uint32_t call_no = 0;
    struct Block {
        ResampBankRun *h = nullptr, *d = nullptr;   // n_streams descriptors, pinned / device
        hipEvent_t read = nullptr;                  // behind the launch that read `d` (and the copy that read `h`)
        bool in_flight = false;
    } blocks[kBankBlocks];
    uint32_t next_block = 0;
    Mixer mix;
    float scale = kInDefaultScale;
    InStat instat;   // input statistics (adsb_instat.cpp), a record per stream: off unless asked for
    Registry mem;   // owns all of the above that the runtime reserved
};

namespace adsb {
namespace host {
MixerOwner mixer_of(adsb_bank *b) { return {b->ctx, &b->mem, &b->mix}; }
float *scale_of(adsb_bank *b) { return &b->scale; }
InStatOwner instat_of(adsb_bank *b) { return {b->ctx, &b->mem, &b->instat, b->n_streams}; }
}  // namespace host
}  // namespace adsb

namespace {

uint32_t *hist_of(const adsb_bank *b, uint32_t stream, int which) { return b->d_hist[which] + (size_t)stream * kResampHistWords; }

bool stream_ok(const adsb_bank *b, uint32_t stream) { return b && stream < b->n_streams; }

// The launch of a call's runs that have input: descriptors, kernels, then the histories' turn and every P.  No wait
// (unless the block's previous user is still in flight).
int run_on_stream(adsb_bank *b, int format, uint32_t n_runs, const uint32_t *streams, const void *const *d_in, const size_t *n_in,
                  void *const *d_out, const size_t *n_out)
{
    adsb_ctx *c = b->ctx;
    adsb_bank::Block &blk = b->blocks[b->next_block];
    if (blk.in_flight) {
        HIP_TRY(c, hipEventSynchronize(blk.read));
        blk.in_flight = false;
    }
    const uint32_t L = b->up, M = b->down;
    ResampParams p{};
    p.u8_table = format == ADSB_DECIM_8BIT ? c->d_u8_table : nullptr;
    p.format = (uint32_t)format;
    p.scale = b->scale;
    filter_params(p, L, M, b->k_taps, b->k_pad, b->shift, b->d_taps);
    p.mix = mixer_params(b->mix, 0);
    uint32_t n = 0;
    for (uint32_t r = 0; r < n_runs; r++) {
        if (!n_in[r]) continue;
        const uint32_t s = streams[r];
        ResampBankRun &d = blk.h[n++];
        d = ResampBankRun{};
        d.src = d_in[r];
        d.n_in = n_in[r];
        d.out = static_cast<uint32_t *>(d_out[r]);
        d.n_out = n_out[r];
        d.hist_prev = hist_of(b, s, b->cur[s]);
        d.hist_next = hist_of(b, s, b->cur[s] ^ 1);
        first_output(L, M, b->consumed[s], &d.p0, &d.q0);
        d.mix_phase = b->mix.period ? (uint32_t)(b->consumed[s] % b->mix.period) : 0u;
        d.reserved = s;   // (k_instat_bank's: the stream whose record the run counts into; k_resamp_bank does not read it)
    }
    if (!n) return ADSB_OK;
    HIP_TRY(c, hipMemcpyAsync(blk.d, blk.h, (size_t)n * sizeof(ResampBankRun), hipMemcpyHostToDevice, c->stream));
    if (c->stream == c->own_stream) c->own_stream_dirty = true;
    // (the raw inputs counted first, from the same descriptors: the block's event below stays behind both launches)
    if (b->instat.on)
        if (int rc = b->instat.count_bank(c, b->instat, b->n_streams, format, b->scale, blk.h, blk.d, n)) return rc;
    if (int e = launch_resamp_bank(p, blk.h, blk.d, n, c->stream)) return fail(c, (hipError_t)e, "launch_resamp_bank");
    HIP_TRY(c, hipEventRecord(blk.read, c->stream));
    blk.in_flight = true;
    b->next_block = (b->next_block + 1) % kBankBlocks;
    for (uint32_t r = 0; r < n_runs; r++) {
        if (!n_in[r]) continue;
        const uint32_t s = streams[r];
        if (b->k_taps > 1) b->cur[s] ^= 1;
        b->consumed[s] += n_in[r];
    }
    return ADSB_OK;
}

}  // namespace

extern "C" {

int adsb_bank_create(adsb_ctx *c, uint32_t n_streams, uint32_t up, uint32_t down, const int16_t *taps, uint32_t n_taps,
                     uint32_t shift, adsb_bank **out)
try {
    if (out) *out = nullptr;
    if (!c || !out || !taps || n_streams < 1 || n_streams > ADSB_MAX_RECEIVERS) return ADSB_ERR_INVALID;
    uint32_t k_taps = 0;
    if (!filter_ok(up, down, taps, n_taps, shift, &k_taps)) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(c);
    adsb_bank *b = new adsb_bank;
    b->ctx = c;
    b->n_streams = n_streams;
    b->up = up, b->down = down, b->n_taps = n_taps, b->k_taps = k_taps, b->k_pad = (k_taps + 7u) & ~7u, b->shift = shift;
    b->cur.assign(n_streams, 0);
    b->consumed.assign(n_streams, 0);
    b->named.assign(n_streams, 0);
    const std::vector<int32_t> pp = polyphase(taps, n_taps, up, b->k_pad);
    const size_t hist_bytes = (size_t)n_streams * kResampHistWords * sizeof(uint32_t);
    const size_t block_bytes = (size_t)n_streams * sizeof(ResampBankRun);
    hipError_t e = b->mem.add(Registry::kDevice, (void **)&b->d_taps, pp.size() * sizeof(int32_t));
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = b->mem.add(Registry::kDevice, (void **)&b->d_hist[k], hist_bytes);
    for (uint32_t k = 0; k < kBankBlocks && e == hipSuccess; k++) {
        adsb_bank::Block &blk = b->blocks[k];
        e = b->mem.add(Registry::kPinned, (void **)&blk.h, block_bytes);
        if (e == hipSuccess) e = b->mem.add(Registry::kDevice, (void **)&blk.d, block_bytes);
        if (e == hipSuccess) e = b->mem.add(Registry::kEvent, (void **)&blk.read, hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipMemcpy(b->d_taps, pp.data(), pp.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipMemset(b->d_hist[k], 0, hist_bytes);
    if (e != hipSuccess) {
        const int rc = e == hipErrorOutOfMemory ? ADSB_ERR_NOMEM : fail(c, e, "adsb_bank_create");
        adsb_bank_destroy(b);
        return rc;
    }
    *out = b;
    return ADSB_OK;
} ADSB_ABI_CATCH

void adsb_bank_destroy(adsb_bank *b)
{
    if (!b) return;
    {
        DeviceGuard guard(b->ctx->device);
        // (what the bank put on the stream may still read its buffers)
        (void)hipStreamSynchronize(b->ctx->stream);
        b->mem.release_all();
    }
    delete b;
}

uint32_t adsb_bank_streams(const adsb_bank *b) { return b ? b->n_streams : 0; }

int adsb_bank_reset(adsb_bank *b, uint32_t stream)
try {
    if (!b || (stream != ADSB_BANK_ALL && stream >= b->n_streams)) return ADSB_ERR_INVALID;
    adsb_ctx *c = b->ctx;
    ADSB_ON_DEVICE(c);
    const uint32_t lo = stream == ADSB_BANK_ALL ? 0 : stream, hi = stream == ADSB_BANK_ALL ? b->n_streams : stream + 1;
    if (hi - lo > 1) {
        // every stream: both allocations whole, two commands whatever N
        const size_t bytes = (size_t)b->n_streams * kResampHistWords * sizeof(uint32_t);
        for (int k = 0; k < 2; k++) HIP_TRY(c, hipMemsetAsync(b->d_hist[k], 0, bytes, c->stream));
    } else {
        HIP_TRY(c, hipMemsetAsync(hist_of(b, lo, b->cur[lo]), 0, kResampHistWords * sizeof(uint32_t), c->stream));
    }
    for (uint32_t s = lo; s < hi; s++) b->consumed[s] = 0;
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_bank_consumed(const adsb_bank *b, uint32_t stream, uint64_t *consumed)
{
    if (!stream_ok(b, stream) || !consumed) return ADSB_ERR_INVALID;
    *consumed = b->consumed[stream];
    return ADSB_OK;
}

int adsb_bank_out_count(const adsb_bank *b, uint32_t stream, size_t n_in, size_t *n_out)
{
    if (!stream_ok(b, stream) || !n_out) return ADSB_ERR_INVALID;
    *n_out = (size_t)out_count(b->up, b->down, b->consumed[stream], n_in);
    return ADSB_OK;
}

int adsb_bank_inputs_for(const adsb_bank *b, uint32_t stream, size_t n_out_wanted, size_t *n_in, size_t *n_out_made)
{
    // (the counts stay within 64 bits: streams of less than 2^56 samples, as adsb_resamp_plan's)
    if (!stream_ok(b, stream) || !n_in || !n_out_made || (uint64_t)n_out_wanted >> 56) return ADSB_ERR_INVALID;
    const uint64_t P = b->consumed[stream];
    const uint64_t n = n_out_wanted ? inputs_for(b->up, b->down, P, n_out_wanted) : 0;
    *n_in = (size_t)n;
    *n_out_made = (size_t)out_count(b->up, b->down, P, n);
    return ADSB_OK;
}

int adsb_bank_run_device(adsb_bank *b, int format, uint32_t n_runs, const uint32_t *streams, const void *const *device_in,
                         const size_t *n_in, void *const *device_out_cs16, const size_t *out_cap, size_t *n_out)
try {
    if (!b || !format_ok(format)) return ADSB_ERR_INVALID;
    if (n_runs == 0) return ADSB_OK;
    if (!streams || !device_in || !n_in || !device_out_cs16 || !out_cap || !n_out || n_runs > b->n_streams) return ADSB_ERR_INVALID;
    if (++b->call_no == 0) {   // (the stamps start over)
        std::fill(b->named.begin(), b->named.end(), 0u);
        b->call_no = 1;
    }
    for (uint32_t r = 0; r < n_runs; r++) {
        const uint32_t s = streams[r];
        if (s >= b->n_streams || b->named[s] == b->call_no) return ADSB_ERR_INVALID;
        b->named[s] = b->call_no;
        if (((uintptr_t)device_in[r] & 15u) != 0 || ((uintptr_t)device_out_cs16[r] & 15u) != 0) return ADSB_ERR_INVALID;
        if (!device_in[r] && n_in[r]) return ADSB_ERR_INVALID;
    }
    bool fits = true, has_out = true;
    for (uint32_t r = 0; r < n_runs; r++) {
        const uint64_t n = out_count(b->up, b->down, b->consumed[streams[r]], n_in[r]);
        n_out[r] = (size_t)n;
        fits = fits && n <= out_cap[r];
        has_out = has_out && (!n || device_out_cs16[r]);
    }
    if (!fits) return ADSB_ERR_CAPACITY;   // nothing consumed
    if (!has_out) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(b->ctx);
    return run_on_stream(b, format, n_runs, streams, device_in, n_in, device_out_cs16, n_out);
} ADSB_ABI_CATCH

uint32_t adsb_bank_get_mixer(const adsb_bank *b) { return b ? b->mix.period : 0; }
float adsb_bank_get_scale(const adsb_bank *b) { return b ? b->scale : 0.0f; }

uint32_t adsb_bank_selftest_depth(void) { return kBankBlocks; }

}  // extern "C"
