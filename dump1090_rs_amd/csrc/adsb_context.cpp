// adsb_context.cpp -- context lifetime, the registry, the stream pool, settings and diagnostics (include/adsb_hip.h).
//
// The functions of the library mirror the reference's library API for the path (src/utils.rs:43 to_mag,
// src/demod_2400.rs:115 demodulate2400, src/icao_filter.rs:11 icao_flush); what each one replaces is
// listed in the header.
#include "adsb_ctx.h"

using namespace adsb::host;

extern "C" {

// Streams.  The runtime multiplexes streams onto hardware queues: GPU_MAX_HW_QUEUES (4 by default) per priority, gives
// every new stream of a priority a new queue until it has four of that priority, never gives one back, and streams
// beyond that SHARE queues, i.e. run one after the other.  Measured in earlier rounds: a process that creates, destroys
// and re-creates contexts ends up with its streams on a different set of queues each time (a dense stream in the second
// context alternated 88 / 270 us per pass); a process with a large context (two scan streams) AND contexts for passes of
// a few buffers (four) held six high-priority streams, two of which shared a queue -- the one-buffer ring ran at 6.8
// instead of 8.8 Gsample/s, or the large stream at 0.129 instead of 0.097 ms per step, depending on who came first --
// unless the process set GPU_MAX_HW_QUEUES=8 before the runtime started.
// So the library never holds more than four streams of a priority per device, whatever its users create
// (profiles/r5_stream_pool_ab.txt).  Per device, for the life of the process:
//   * TWO highest-priority streams that every large context's scans alternate between.  Exactly two: with four in
//     existence -- even unused -- the large sparse stream's step went from 0.096 to 0.125 ms (consecutive scans no
//     longer overlapped);
//   * FOUR normal-priority streams, made when the first context for passes of a few buffers is, that every such
//     context's one-launch passes rotate over: 10.3-10.6 Gsample/s for the one-buffer ring in a process of its own
//     (four high-priority ones of its own, round 4: 8.7 on the same box; the two shared high-priority ones alone: 8.9;
//     two high + two normal: 6.3 -- mixed priorities finish passes out of order);
//   * TWO lowest-priority ones for the contexts' tail and score chains.
// Contexts that share a stream are simply several in-order users of it (every wait is for an event recorded before it
// was asked for: no cycle).  No environment variable is needed by anybody.
struct DeviceStreams {
    int device = -1;
    int least = 0, greatest = 0;
    hipStream_t high[2] = {};              // highest priority: the scans of large contexts
    hipStream_t small[kScanStreams] = {};  // the four scan streams of contexts for passes of a few buffers
    hipStream_t low[4] = {};               // lowest priority: tail and score chains
    int n_low = 0;
    unsigned next_low = 0;
    std::vector<hipStream_t> free_own;     // normal priority: a context's own stream (input order, host-pointer copies)
};
std::mutex g_streams_mu;
// (never freed, not even at exit, so that leak checkers see the pools as reachable: the streams live as long as the process)
std::vector<DeviceStreams *> &g_device_streams = *new std::vector<DeviceStreams *>;

// A stream with a hardware queue of its own.  The runtime maps the streams of a process onto at most four hardware queues
// per priority (GPU_MAX_HW_QUEUES): the fifth stream of a priority shares the queue of an earlier one -- whichever has the
// fewest users at that moment -- and two streams on one queue run their work in order.  Which of the library's streams
// ended up sharing therefore depended on how many streams of that priority the HOST had made before (torch's null stream,
// the contexts' own streams): the four scan streams of a context for passes of a few buffers came out as two, three or
// four queues, and the one-buffer ring ran at 9.0, 10.8 or 11.5 Gsample/s (profiles/r6_stream_queues.txt).  A stream
// created with a CU mask never enters that pool -- the runtime gives it a queue of its own -- and a mask with every CU
// enabled restricts nothing.
hipError_t dedicated_stream(int device, hipStream_t *out)
{
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return e;
    std::vector<uint32_t> mask((size_t)(prop.multiProcessorCount + 31) / 32, 0xFFFFFFFFu);
    if (prop.multiProcessorCount % 32) mask.back() = (1u << (prop.multiProcessorCount % 32)) - 1u;
    return hipExtStreamCreateWithCUMask(out, (uint32_t)mask.size(), mask.data());
}

// under g_streams_mu, the device current.  Every stream is made where it is still missing, so a call that failed halfway
// is completed by the next one.
int device_streams(adsb_ctx *c, int device, bool small, DeviceStreams **out)
{
    DeviceStreams *d = nullptr;
    for (DeviceStreams *e : g_device_streams)
        if (e->device == device) d = e;
    if (!d) {
        int least = 0, greatest = 0;
        HIP_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        g_device_streams.reserve(g_device_streams.size() + 1);
        d = new (std::nothrow) DeviceStreams;
        if (!d) return ADSB_ERR_NOMEM;
        d->device = device, d->least = least, d->greatest = greatest;
        g_device_streams.push_back(d);
    }
    // The two scan streams take the highest priority: that pool holds nothing else of this process (the null stream,
    // torch's and the caller's streams are of normal priority), so each gets a queue and consecutive scans overlap.
    // They must have the SAME priority: with different ones, whenever two scans are pending at once the higher one
    // starts first, its successor on that stream is then free earlier too, and the stream settles into finishing
    // passes in the order 2, 1, 4, 3, ... for thousands of passes, 8-10 % slower (measured over 22 000 passes).
    // (measurement aid, tuning builds: ADSB_POOL_LARGE=1 the two scan streams of large contexts with a hardware queue each
    // instead of the highest priority, =2 the tail and score streams as well)
    const int large_variant = tuning_env("ADSB_POOL_LARGE") ? std::atoi(tuning_env("ADSB_POOL_LARGE")) : 0;
    for (auto &q : d->high) {
        if (q) continue;
        if (large_variant >= 1) HIP_TRY(c, dedicated_stream(device, &q));
        else HIP_TRY(c, hipStreamCreateWithPriority(&q, hipStreamNonBlocking, d->greatest));
    }
    if (!d->n_low) {
        const int n = 2;
        for (int k = 0; k < 4; k++) {
            if (k >= n) d->low[k] = d->low[k % n];
            else if (d->low[k]) continue;
            else if (large_variant >= 2) HIP_TRY(c, dedicated_stream(device, &d->low[k]));
            else HIP_TRY(c, hipStreamCreateWithPriority(&d->low[k], hipStreamNonBlocking, d->least));
        }
        d->n_low = n;
    }
    if (small) {
        // (measurement aid, tuning builds: 0 the two high-priority streams + two more, 1 those two + two of normal
        // priority, 2 four of normal priority, 3 four high-priority ones of its own, 4 four of the lowest priority,
        // 5 four streams with a hardware queue each: hipExtStreamCreateWithCUMask, every CU enabled)
        const int variant = tuning_env("ADSB_POOL_SMALL") ? std::atoi(tuning_env("ADSB_POOL_SMALL")) : 5;
        const int mid = (d->least + d->greatest) / 2;
        for (int k = 0; k < kScanStreams; k++) {
            if (d->small[k]) continue;
            const bool share = (variant == 0 || variant == 1) && k < 2;
            const int prio = variant == 0 || variant == 3 ? d->greatest : (variant == 4 ? d->least : mid);
            if (share) d->small[k] = d->high[k];
            else if (variant == 5) {
                // (a runtime that refuses the mask: the pool stream this used to be -- slower when the host's own streams
                // crowd the pool, never wrong)
                if (dedicated_stream(device, &d->small[k]) != hipSuccess) {
                    (void)hipGetLastError();
                    HIP_TRY(c, hipStreamCreateWithPriority(&d->small[k], hipStreamNonBlocking, mid));
                }
            }
            else HIP_TRY(c, hipStreamCreateWithPriority(&d->small[k], hipStreamNonBlocking, prio));
        }
    }
    *out = d;
    return ADSB_OK;
}

}  // extern "C"

// ---- the registry (adsb_ctx.h) ----
static void free_entry(const Registry::Entry &en)
{
    if (en.kind == Registry::kDevice) (void)hipFree(en.p);
    else if (en.kind == Registry::kPinned) (void)hipHostFree(en.p);
    else (void)hipEventDestroy(static_cast<hipEvent_t>(en.p));
    *en.home = nullptr;
}

// (the entry first: a reservation the vector has no room for is never made, so none is ever without its entry)
hipError_t Registry::add(Kind kind, void **home, size_t arg)
{
    entries.push_back({kind, nullptr, home});
    void *&p = entries.back().p;
    const hipError_t e = kind == kDevice   ? hipMalloc(&p, arg)
                         : kind == kPinned ? hipHostMalloc(&p, arg, hipHostMallocMapped | hipHostMallocCoherent)
                                           : hipEventCreateWithFlags(reinterpret_cast<hipEvent_t *>(&p), (unsigned)arg);
    if (e != hipSuccess) entries.pop_back();
    else *home = p;
    return e;
}

void Registry::release(void **home)
{
    for (size_t k = entries.size(); k-- > 0;)
        if (entries[k].home == home) {
            free_entry(entries[k]);
            entries.erase(entries.begin() + (long)k);
            return;
        }
}

void Registry::release_from(size_t mark)
{
    for (; entries.size() > mark; entries.pop_back()) free_entry(entries.back());
}

// ---- adsb_create, step by step (in this order; adsb_destroy undoes whatever a failed step leaves) ----
namespace {

// How many passes in flight, streams and list entries a context of c->max_chunks buffers gets (the device is current).
void size_lists(adsb_ctx *c)
{
    const size_t max_chunks = c->max_chunks;
    // (a context for passes of a few buffers: one launch each, eight in flight -- adsb_ctx.h)
    c->n_slots = max_chunks <= kInlineTailChunks ? ADSB_MAX_IN_FLIGHT_SMALL : ADSB_MAX_IN_FLIGHT;
    c->n_bitmaps = c->n_slots + 1;
    c->n_scan_streams = c->n_slots == ADSB_MAX_IN_FLIGHT_SMALL ? kScanStreams : 2;
    c->bitmap_lg = c->n_slots == ADSB_MAX_IN_FLIGHT_SMALL ? kSmallBitmapLg : kFullBitmapLg;
    if (const char *ds = tuning_env("ADSB_DEBUG_STOP")) c->debug_stop = std::atoi(ds);
    if (const char *st = tuning_env("ADSB_STAGGER")) c->stagger_ticks = (uint32_t)std::atoi(st);
    // The fast scan's AP list: one private segment per wave of every persistent workgroup (a pass
    // of n buffers runs min(17 n, resident grid) workgroups of four waves, so a small context only gets
    // the segments it can ever use), each sized for ~5x the rate pure noise produces (2.3 % of
    // samples become address/parity entries).  Denser input falls back to buffer-by-buffer
    // passes through the reference-shaped kernel, whose list (dap) and the hit list hold one
    // buffer's worst case: every position sliced, five trials each.
    const uint64_t used_segs = 4 * std::min<uint64_t>((uint64_t)scan_resident_blocks(), max_chunks * (uint64_t)fastgeo::kTilesPerChunk);
    c->seg_cap = (uint32_t)std::max<uint64_t>(1024, (max_chunks * (uint64_t)kChunkSamples / 8 + used_segs - 1) / used_segs);
    c->ap_cap = (uint32_t)(used_segs * c->seg_cap);
    // hit list: ~5x what a busy airspace produces (a frame leaves 3-4 trial records; 1000 frames/s
    // are ~55 per buffer); more than that is the fallback's business too
    c->hits_cap = (uint32_t)(4096 + max_chunks * 1024);
    // device-side scoring (shared by the passes: they go through it one after the other on the tail stream); passes of
    // more hits than `cap` are scored on the host.  A context for passes of a few buffers never orders or scores on the
    // device -- its passes are one launch each, replayed by the host in microseconds -- and carries none of it: no exact
    // bitmaps, no scoring buffers, no message slots in its pinned block.
    ScoreDev &cd = c->score;   // cap / hash_mask / exact: the context's; the rest per slot
    const bool scoring = c->n_slots != ADSB_MAX_IN_FLIGHT_SMALL;
    cd.cap = scoring ? std::min<uint32_t>(c->hits_cap, 262144u) : 0u;   // (a 2 GiB shard of a busy sky leaves 135 000)
    cd.hash_mask = score_hash_size(cd.cap) - 1;
}

int take_streams(adsb_ctx *c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (tuning_env("ADSB_STREAM_PRIO") || tuning_env("ADSB_SCORE_PRIO")) {
        // measurement aid (tuning builds): streams of this context's own, "tail,scan0,scan1" as 0 (least) .. 2
        int least = 0, greatest = 0;
        HIP_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        int pt = least, p0 = greatest, p1 = greatest, ps = least;
        if (const char *e = tuning_env("ADSB_STREAM_PRIO")) {
            int a = 0, b = 1, d = 2;
            if (std::sscanf(e, "%d,%d,%d", &a, &b, &d) == 3) {
                const int lv[3] = {least, (least + greatest) / 2, greatest};
                pt = lv[a % 3], p0 = lv[b % 3], p1 = lv[d % 3];
            }
        }
        if (const char *e = tuning_env("ADSB_SCORE_PRIO")) ps = std::atoi(e) == 2 ? greatest : (std::atoi(e) == 1 ? (least + greatest) / 2 : least);
        c->private_streams = true;
        HIP_TRY(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        HIP_TRY(c, hipStreamCreateWithPriority(&c->tail_stream, hipStreamNonBlocking, pt));
        for (int k = 0; k < c->n_scan_streams; k++) HIP_TRY(c, hipStreamCreateWithPriority(&c->scan_stream[k], hipStreamNonBlocking, k & 1 ? p1 : p0));
        HIP_TRY(c, hipStreamCreateWithPriority(&c->score_stream, hipStreamNonBlocking, ps));
    } else {
        std::lock_guard<std::mutex> lk(g_streams_mu);
        DeviceStreams *ds = nullptr;
        const bool small = c->n_scan_streams == kScanStreams;
        if (int rc = device_streams(c, c->device, small, &ds)) return rc;
        for (int k = 0; k < c->n_scan_streams; k++) c->scan_stream[k] = small ? ds->small[k] : ds->high[k];
        c->tail_stream = ds->low[ds->next_low++ & 3u];
        c->score_stream = ds->low[ds->next_low++ & 3u];
        if (!ds->free_own.empty()) {
            c->own_stream = ds->free_own.back();
            ds->free_own.pop_back();
        } else {
            HIP_TRY(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        }
    }
    c->stream = c->own_stream;
    return ADSB_OK;
}

// The address supersets, every slot's device lists (zero where a pass expects zero), and the events.
int reserve_lists_and_events(adsb_ctx *c)
{
    const size_t max_chunks = c->max_chunks;
    for (auto &e : c->input_ready) HIP_TRY(c, new_event(c, &e, kQuietEvent));
    HIP_TRY(c, new_event(c, &c->lazy_ev, kQuietEvent));
    for (int k = 0; k < c->n_bitmaps; k++) HIP_TRY(c, dev_alloc(c, &c->d_bitmap[k], bitmap_alloc_words(c->bitmap_lg) * sizeof(uint32_t)));
    const bool fenced = tuning_env("ADSB_DONE_FENCE") != nullptr;  // measurement aid only
    for (int si = 0; si < c->n_slots; si++) {
        Slot &sl = c->slot[si];
        sl.hits_cap = c->hits_cap;
        const size_t cnt_bytes = (max_chunks * fastgeo::kTilesPerChunk + 1) * sizeof(uint32_t);
        HIP_TRY(c, dev_alloc(c, &sl.d_ctr, sizeof(Counters)));
        HIP_TRY(c, dev_alloc(c, &sl.d_hits, (size_t)c->hits_cap * sizeof(uint64_t)));
        HIP_TRY(c, dev_alloc(c, &sl.d_hit_fields, (size_t)c->hits_cap * kHitFieldWords * sizeof(uint32_t)));
        HIP_TRY(c, dev_alloc(c, &sl.d_ap, (size_t)c->ap_cap * sizeof(uint64_t)));
        HIP_TRY(c, dev_alloc(c, &sl.d_order_cnt, cnt_bytes));
        HIP_TRY(c, hipMemset(sl.d_order_cnt, 0, cnt_bytes));
        HIP_TRY(c, dev_alloc(c, &sl.d_order_base, (max_chunks + 1) * sizeof(uint32_t)));
        HIP_TRY(c, dev_alloc(c, &sl.d_order_tmp, (size_t)c->hits_cap * sizeof(uint64_t)));
        HIP_TRY(c, dev_alloc(c, &sl.d_carry, kCarrySamples * sizeof(uint32_t)));
        HIP_TRY(c, hipMemset(sl.d_carry, 0, kCarrySamples * sizeof(uint32_t)));
        HIP_TRY(c, new_event(c, &sl.scanned, kQuietEvent));
        HIP_TRY(c, new_event(c, &sl.recorded, kQuietEvent));
        // timing-only events: no system-scope fence when they complete (~10 us each otherwise)
        for (int k = 2; k < 5; k++) HIP_TRY(c, new_event(c, &sl.ev[k], hipEventDisableSystemFence));
        // (the slot's summary and records live in the context's one pinned block: mapped + coherent, so the records
        // kernel's write-through stores are visible to the host when its completion event fires)
        HIP_TRY(c, new_event(c, &sl.done, fenced ? hipEventDisableTiming : kQuietEvent));
    }
    HIP_TRY(c, dev_alloc(c, &c->d_carry_next, kCarrySamples * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(c->d_carry_next, 0, kCarrySamples * sizeof(uint32_t)));
    for (auto &pair : c->scan_ev)
        for (auto &e : pair) HIP_TRY(c, new_event(c, &e, hipEventDisableSystemFence));
    for (auto &e : c->redo_ev) HIP_TRY(c, new_event(c, &e, hipEventDisableSystemFence));
    if (tuning_env("ADSB_TIMELINE")) {
        // 1: stamps of 8 blocks x 8 tiles; 2 (with ADSB_DEBUG_STOP=100): per-wave phase totals
        HIP_TRY(c, dev_alloc(c, &c->d_timeline, kTimelineWords * sizeof(unsigned long long)));
        HIP_TRY(c, hipMemset(c->d_timeline, 0, kTimelineWords * sizeof(unsigned long long)));
    }
    return ADSB_OK;
}

// The two exact bitmaps and every slot's scoring buffers (a context that scores on the device: size_lists).
int reserve_scoring(adsb_ctx *c)
{
    ScoreDev &cd = c->score;
    if (cd.cap) {
        for (auto &bm : c->exact_bm) {
            HIP_TRY(c, dev_alloc(c, &bm, kBitmapAllocWords * sizeof(uint32_t)));
            HIP_TRY(c, hipMemset(bm, 0, kBitmapAllocWords * sizeof(uint32_t)));
        }
        cd.exact = c->exact_bm[0];
        cd.si = reinterpret_cast<uint32_t *>(cd.exact);  // (non-null: "scoring is available")
    }
    const size_t hsize = (size_t)cd.hash_mask + 1;
    for (int si = 0; si < c->n_slots; si++) {
        ScoreDev &sd = c->slot[si].score;
        sd = cd;
        if (!cd.cap) continue;
        HIP_TRY(c, dev_alloc(c, &sd.si, (size_t)sd.cap * sizeof(uint32_t)));
        HIP_TRY(c, dev_alloc(c, &sd.rec, (size_t)sd.cap * sizeof(TrialRecord)));
        HIP_TRY(c, dev_alloc(c, &sd.flag, (size_t)sd.cap * sizeof(uint32_t)));
        HIP_TRY(c, dev_alloc(c, &sd.pos, (size_t)sd.cap * sizeof(unsigned long long)));
        HIP_TRY(c, dev_alloc(c, &sd.slot, (size_t)sd.cap * sizeof(uint32_t)));
        HIP_TRY(c, dev_alloc(c, &sd.hash, hsize * sizeof(unsigned long long)));
        HIP_TRY(c, hipMemset(sd.hash, 0xFF, hsize * sizeof(unsigned long long)));
        HIP_TRY(c, dev_alloc(c, &sd.blk, 2 * kScoreBlocks * sizeof(uint32_t)));
        HIP_TRY(c, dev_alloc(c, &sd.state, sizeof(ScoreState)));
        HIP_TRY(c, hipMemset(sd.state, 0, sizeof(ScoreState)));
    }
    return ADSB_OK;
}

// The host side of every slot -- summary, score summary, additions, records, messages: mapped, coherent, written by the
// kernels with write-through stores -- as ONE pinned allocation per context, cut up here.
// (five separate allocations per slot were forty small pinned regions in a one-buffer context)
int carve_host_block(adsb_ctx *c)
{
    const size_t cap = c->score.cap;
    const size_t o_ssum = up256(sizeof(Summary)), o_adds = o_ssum + up256(sizeof(ScoreSummary)),
                 o_rec = o_adds + up256(cap * sizeof(uint32_t)), o_msgs = o_rec + up256((size_t)c->hits_cap * sizeof(TrialRecord)),
                 per_slot = o_msgs + up256(cap * sizeof(adsb_msg));
    HIP_TRY(c, pinned_alloc(c, &c->h_block, &c->h_block_dev, per_slot * (size_t)c->n_slots));
    for (int si = 0; si < c->n_slots; si++) {
        Slot &sl = c->slot[si];
        char *h = c->h_block + per_slot * (size_t)si, *d = c->h_block_dev + per_slot * (size_t)si;
        sl.h_sum = reinterpret_cast<Summary *>(h), sl.h_sum_dev = reinterpret_cast<Summary *>(d);
        sl.h_ssum = reinterpret_cast<ScoreSummary *>(h + o_ssum), sl.h_ssum_dev = reinterpret_cast<ScoreSummary *>(d + o_ssum);
        sl.h_adds = reinterpret_cast<uint32_t *>(h + o_adds), sl.h_adds_dev = reinterpret_cast<uint32_t *>(d + o_adds);
        sl.h_rec = reinterpret_cast<TrialRecord *>(h + o_rec), sl.h_rec_dev = reinterpret_cast<TrialRecord *>(d + o_rec);
        sl.h_msgs = reinterpret_cast<adsb_msg *>(h + o_msgs), sl.h_msgs_dev = reinterpret_cast<adsb_msg *>(d + o_msgs);
        std::memset(sl.h_sum, 0, sizeof(Summary));
        std::memset(sl.h_ssum, 0, sizeof(ScoreSummary));
    }
    return ADSB_OK;
}

// The kernels' lookup tables and the CU8 widening table, built on the host and copied once.
int upload_tables(adsb_ctx *c)
{
    std::vector<uint32_t> tab = build_gf_tables();
    const std::vector<uint32_t> r16 = build_r16(), ft = build_field_table(fast_plane_bytes()), bits = build_bit_residuals();
    tab.insert(tab.end(), r16.begin(), r16.end());
    tab.insert(tab.end(), ft.begin(), ft.end());
    tab.insert(tab.end(), bits.begin(), bits.end());
    uint32_t fix_mult = 0;
    const std::vector<uint32_t> fix = build_fix_table(&fix_mult);
    tab.insert(tab.end(), fix.begin(), fix.end());
    tab.push_back(fix_mult);
    tab.resize(kTabFix2Off, 0u);
    const std::vector<uint32_t> fix2 = build_fix2_table();
    tab.insert(tab.end(), fix2.begin(), fix2.end());
    HIP_TRY(c, dev_alloc(c, &c->d_tables, kTabWords * sizeof(uint32_t)));
    HIP_TRY(c, hipMemcpy(c->d_tables, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    int16_t t[256];
    soapy_u8_table(t);
    HIP_TRY(c, dev_alloc(c, &c->d_u8_table, 256 * sizeof(uint16_t)));
    HIP_TRY(c, hipMemcpy(c->d_u8_table, t, sizeof t, hipMemcpyHostToDevice));
    return ADSB_OK;
}

// Every bitmap clean and every counter block zero to start with; from then on each pass cleans up for the next (the
// first pass needs no flush of its own).
int initial_resets(adsb_ctx *c)
{
    for (int k = 0; k < c->n_bitmaps; k++)
        if (int e = launch_reset(c->slot[k % (uint64_t)c->n_slots].d_ctr, c->d_bitmap[k], c->bitmap_lg, c->stream))
            return fail(c, (hipError_t)e, "launch_reset");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->flush_pending = false;
    return ADSB_OK;
}

}  // namespace

extern "C" {

int adsb_create(adsb_ctx **out, int device, size_t max_chunks)
try {
    if (!out) return ADSB_ERR_INVALID;
    *out = nullptr;
    if (device < 0) return ADSB_ERR_NO_DEVICE;  // no CPU backend by design
    if (max_chunks == 0) max_chunks = 1;
    if (max_chunks > kMaxChunks) return ADSB_ERR_INVALID;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device >= count) return ADSB_ERR_NO_DEVICE;
    {
        // the kernels are gfx950 code objects and nothing else: any other device is "no usable device" here, not a
        // failed launch later (include/adsb_hip.h: ADSB_ERR_NO_DEVICE)
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return ADSB_ERR_NO_DEVICE;
    }
    DeviceGuard on_device(device);  // (scan_resident_blocks() asks the current device; the caller's is put back on the way out)
    if (on_device.err != hipSuccess) return ADSB_ERR_NO_DEVICE;
    adsb_ctx *c = new (std::nothrow) adsb_ctx;
    if (!c) return ADSB_ERR_NOMEM;
    c->device = device;
    c->max_chunks = max_chunks;
    size_lists(c);
    int rc = ADSB_OK;
    for (auto step : {take_streams, reserve_lists_and_events, reserve_scoring, carve_host_block, upload_tables, initial_resets})
        if (rc == ADSB_OK) rc = step(c);
    if (rc != ADSB_OK) {
        std::fprintf(stderr, "adsb_create: %s\n", c->last_error.c_str());
        adsb_destroy(c);
        return rc;
    }
    *out = c;
    return ADSB_OK;
} ADSB_ABI_CATCH

}  // extern "C"

namespace adsb {
namespace host {

// ---- what a tuning build prints at destroy: the host-times table (ADSB_HOST_TIMES; tools/hosttime.py parses it) and the
// timelines the scan kernels stamp into adsb_ctx::d_timeline (ADSB_TIMELINE) ----
static void print_host_times(const adsb_ctx *c)
{
#ifdef ADSB_TUNING
    if (tuning_env("ADSB_HOST_TIMES")) {
        std::fprintf(stderr, "host times over %llu passes: enqueue %.1f us, wait %.1f us, replay %.1f us per pass\n",
                     (unsigned long long)c->collected, 1e6 * c->t_enqueue / (c->collected ? c->collected : 1),
                     1e6 * c->t_wait / (c->collected ? c->collected : 1), 1e6 * c->t_replay / (c->collected ? c->collected : 1));
        static const char *name[HT_COUNT] = {"ring: hipMemcpyAsync", "ring: (unused)", "input-ready record + wait",
                                             "scan launch", "scanned record + waits", "match (+ order) launch", "records launch",
                                             "recorded / done records", "collect: wait for the pass", "collect: record checksum",
                                             "collect: replay"};
        double all = 0;
        for (int k = 0; k < HT_COUNT; k++) all += c->ht_s[k];
        for (int k = 0; k < HT_COUNT; k++)
            if (c->ht_n[k])
                std::fprintf(stderr, "  %-32s %8.2f us per pass  (%llu calls, %.2f us each)  %5.1f %%\n", name[k],
                             1e6 * c->ht_s[k] / (c->collected ? c->collected : 1), (unsigned long long)c->ht_n[k],
                             1e6 * c->ht_s[k] / c->ht_n[k], 100.0 * c->ht_s[k] / (all > 0 ? all : 1));
    }
#endif
    (void)c;
}

// ADSB_TIMELINE=3: the stamps of the last one-launch pass (100 MHz wall clock)
static void dump_onelaunch_timeline(const adsb_ctx *c)
{
    unsigned long long t[10] = {};
    if (hipMemcpy(t, c->d_timeline + 448, sizeof(t), hipMemcpyDeviceToHost) == hipSuccess && t[0]) {
        if (t[8] > t[4] && t[7] > t[8])
            std::fprintf(stderr, "  one-launch pass, second look: fill counts in LDS +%.2f us, entries compared +%.2f us, fence +%.2f us\n",
                         (double)(long long)(t[8] - t[4]) / 100.0, (double)(long long)(t[7] - t[8]) / 100.0,
                         (double)(long long)(t[5] - t[7]) / 100.0);
        static const char *name[7] = {"entry", "tables in LDS, first tile requested", "tiles done", "own entries matched",
                                      "counted in (last workgroup from here on)", "second look done", "records + summary + counters"};
        for (int k = 1; k < 7; k++)
            std::fprintf(stderr, "  one-launch pass: %-45s +%6.2f us  (at %6.2f)\n", name[k],
                         (double)(long long)(t[k] - t[k - 1]) / 100.0, (double)(long long)(t[k] - t[0]) / 100.0);
    }
    // ... and of the last sixteen, workgroup by workgroup: when the first and the last workgroup passed each
    // stage, from the pass's first entry (passes in flight side by side: how they stretch each other)
    std::vector<unsigned long long> w(16 * 32 * 8);
    if (hipMemcpy(w.data(), c->d_timeline + 1024, w.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
        unsigned long long origin = ~0ull;
        for (unsigned long long v : w) if (v && v < origin) origin = v;
        for (int ps = 0; ps < 16; ps++) {
            unsigned long long lo[8], hi[8] = {};
            for (auto &v : lo) v = ~0ull;
            for (int g = 0; g < 32; g++)
                for (int k = 0; k < 8; k++) {
                    const unsigned long long v = w[(ps * 32 + g) * 8 + k];
                    if (!v) continue;
                    lo[k] = std::min(lo[k], v);
                    hi[k] = std::max(hi[k], v);
                }
            if (!hi[0]) continue;
            std::fprintf(stderr, "  pass %2d entered at %8.2f us:", ps, (double)(lo[0] - origin) / 100.0);
            for (int k = 0; k < 7; k++)
                if (hi[k]) std::fprintf(stderr, "  s%d %.1f..%.1f", k, (double)(lo[k] - lo[0]) / 100.0, (double)(hi[k] - lo[0]) / 100.0);
            std::fprintf(stderr, "\n");
        }
    }
}

// ADSB_DEBUG_STOP=100: phase / barrier-wait totals of the last scan, summed over all waves
static void dump_scan_phases(const adsb_ctx *c)
{
    std::vector<unsigned long long> tl(kTimelineWords);
    if (hipMemcpy(tl.data(), c->d_timeline, kTimelineWords * 8, hipMemcpyDeviceToHost) == hipSuccess) {
        double sum[8] = {0};
        int nw = 0;
        for (size_t w = 0; w < kTimelineWords / 8; w++) {
            double tot = 0;
            for (int k = 0; k < 8; k++) tot += (double)tl[w * 8 + k];
            if (tot == 0) continue;
            nw++;
            for (int k = 0; k < 8; k++) sum[k] += (double)tl[w * 8 + k];
        }
        double all = 0;
        for (double v : sum) all += v;
        static const char *name[8] = {"P1", "wait B1", "P2", "wait B2", "P3-5", "wait B3", "epilogue", "wait B4"};
        std::fprintf(stderr, "phase accounting over %d waves (clock64 ticks per wave, share):\n", nw);
        for (int k = 0; k < 8; k++)
            std::fprintf(stderr, "  %-9s %10.0f  %5.1f %%\n", name[k], sum[k] / (nw ? nw : 1), 100.0 * sum[k] / (all ? all : 1));
        // ... and how evenly the work fell: a workgroup's total (its waves agree to a barrier wait) and its
        // wave-private stage, over the workgroups -- the launch ends with the slowest one
        std::vector<double> tot, late;
        for (size_t w = 0; w + 3 < kTimelineWords / 8; w += 4) {
            double t = 0, l = 0;
            for (int k = 0; k < 8; k++) t += (double)tl[w * 8 + k];
            for (size_t v = 0; v < 4; v++) l = std::max(l, (double)tl[(w + v) * 8 + 4]);
            if (t == 0) continue;
            tot.push_back(t);
            late.push_back(l);
        }
        auto pct = [](std::vector<double> &v, double q) { std::sort(v.begin(), v.end()); return v.empty() ? 0.0 : v[(size_t)(q * (double)(v.size() - 1))]; };
        double mt = 0, ml = 0;
        for (double v : tot) mt += v;
        for (double v : late) ml += v;
        mt /= tot.empty() ? 1 : (double)tot.size();
        ml /= late.empty() ? 1 : (double)late.size();
        std::fprintf(stderr, "  per workgroup (wave 0's total): mean %.0f  p50 %.0f  p99 %.0f  max %.0f  (max / mean %.3f)\n", mt, pct(tot, 0.5),
                     pct(tot, 0.99), pct(tot, 1.0), mt > 0 ? pct(tot, 1.0) / mt : 0.0);
        std::fprintf(stderr, "  per workgroup (its slowest wave's P3-5): mean %.0f  p50 %.0f  p99 %.0f  max %.0f  (max / mean %.3f)\n", ml,
                     pct(late, 0.5), pct(late, 0.99), pct(late, 1.0), ml > 0 ? pct(late, 1.0) / ml : 0.0);
    }
}

// otherwise: the stamps of the last scan
static void dump_scan_stamps(const adsb_ctx *c)
{
    unsigned long long tl[512];
    if (hipMemcpy(tl, c->d_timeline, sizeof(tl), hipMemcpyDeviceToHost) == hipSuccess)
        for (int b = 0; b < 8; b++)
            for (int it = 0; it < 8; it++) {
                const unsigned long long *r = tl + (b * 8 + it) * 8;
                if (!r[0]) continue;
                std::fprintf(stderr, "timeline block %d tile %d: start %8lld |", b * 128, it,
                             (long long)(r[0] - tl[0]));
                for (int k = 1; k < 7; k++) std::fprintf(stderr, " %6lld", (long long)(r[k] - r[k - 1]));
                std::fprintf(stderr, "  total %lld\n", (long long)(r[6] - r[0]));
            }
}

// Signal statistics: per pass in flight max_chunks records in mapped host memory (written once each by k_signal_stats)
// and as many partials plus a ticket per buffer in device memory, zero between passes.  Reserved the first time the mode
// is enabled, so that a context that never enables it keeps the footprint include/adsb_hip.h documents.
int ensure_signal_stats(adsb_ctx *c)
{
    if (c->d_sig_block) return ADSB_OK;   // (reserved last)
    const size_t rec_bytes = up256(c->max_chunks * sizeof(adsb_signal_stats));
    const size_t part_words = c->max_chunks * (size_t)kSigRecordWords, slot_words = (part_words + c->max_chunks + 63) & ~(size_t)63;
    Rollback undo{c->mem, c->mem.mark(), false};
    HIP_TRY(c, pinned_alloc(c, &c->h_sig_block, &c->h_sig_block_dev, rec_bytes * (size_t)c->n_slots));
    HIP_TRY(c, dev_alloc(c, &c->d_sig_block, slot_words * (size_t)c->n_slots * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(c->d_sig_block, 0, slot_words * (size_t)c->n_slots * sizeof(uint32_t)));
    undo.keep = true;
    for (int si = 0; si < c->n_slots; si++) {
        Slot &sl = c->slot[si];
        sl.h_sig = reinterpret_cast<adsb_signal_stats *>(c->h_sig_block + rec_bytes * (size_t)si);
        sl.h_sig_dev = reinterpret_cast<adsb_signal_stats *>(c->h_sig_block_dev + rec_bytes * (size_t)si);
        sl.d_sig_part = c->d_sig_block + slot_words * (size_t)si;
        sl.d_sig_ticket = sl.d_sig_part + part_words;
    }
    return ADSB_OK;
}

// The worst-case lists of the buffer-by-buffer fallback (adsb_ctx::Fallback), the first time a pass overflows.
int ensure_fallback(adsb_ctx *c)
{
    auto &fb = c->fb;
    if (fb.h_rec) return ADSB_OK;   // (reserved last)
    Rollback undo{c->mem, c->mem.mark(), false};
    HIP_TRY(c, dev_alloc(c, &fb.d_hits, (size_t)kWorstPerChunk * sizeof(uint64_t)));
    HIP_TRY(c, dev_alloc(c, &fb.d_dap, (size_t)kWorstPerChunk * sizeof(uint64_t)));
    HIP_TRY(c, pinned_alloc(c, &fb.h_rec, &fb.h_rec_dev, (size_t)kWorstPerChunk * sizeof(TrialRecord)));
    return undo.keep = true, ADSB_OK;
}

// The growers: one buffer each, replaced by a larger one when a call needs more.  The old one goes first (nothing in
// flight reads it, and the two never add up): a failure leaves the buffer absent and its size zero.
template <class T>
static int grow(adsb_ctx *c, T **buf, size_t *have, size_t want, size_t alloc, size_t elem)
{
    if (want <= *have) return ADSB_OK;
    release(c, buf);
    *have = 0;
    HIP_TRY(c, dev_alloc(c, buf, alloc * elem));
    *have = alloc;
    return ADSB_OK;
}
int ensure_stage(adsb_ctx *c, size_t bytes) { return grow(c, &c->d_stage, &c->stage_bytes, bytes, bytes, 1); }
int ensure_addrs(adsb_ctx *c, size_t n, size_t alloc) { return grow(c, &c->d_addrs, &c->addrs_cap, n, alloc, sizeof(uint32_t)); }
int ensure_rx_keys(adsb_ctx *c, size_t n)
{
    return grow(c, &c->d_rx_keys, &c->rx_keys_cap, n, std::max<size_t>(n + n / 2, IcaoFilter::kSize), sizeof(unsigned long long));
}

// pinned, mapped staging for host-pointer calls of a few buffers: the pass reads it in place over the
// link, which saves the copy command and its event
int ensure_host_stage(adsb_ctx *c, size_t bytes)
{
    if (bytes <= c->h_stage_bytes) return ADSB_OK;
    release(c, &c->h_stage);
    c->h_stage_dev = nullptr;
    c->h_stage_bytes = 0;
    HIP_TRY(c, pinned_alloc(c, &c->h_stage, &c->h_stage_dev, bytes));
    c->h_stage_bytes = bytes;
    return ADSB_OK;
}

// CU8 through the overflow fallback: one buffer and its lead-in widened to CS16
int ensure_widen(adsb_ctx *c)
{
    if (!c->d_widen) HIP_TRY(c, dev_alloc(c, &c->d_widen, ((size_t)kChunkSamples + kCarrySamples) * sizeof(uint32_t)));
    return ADSB_OK;
}

// Shard slot k's address lists in mapped host memory: the other shards' addresses (two lists: ShardJob::addr_half) and,
// for a shard whose scan lists its fresh addresses, that list, its seen-set and the earlier shards' additions.
int ensure_shard_lists(adsb_ctx *c, int k, bool fresh_list)
{
    adsb_ctx::ShardJob &job = c->shard[k];
    const size_t list_bytes = kShardAddrCap * sizeof(uint32_t);
    Rollback undo{c->mem, c->mem.mark(), false};
    if (!job.h_addrs) HIP_TRY(c, pinned_alloc(c, &job.h_addrs, &job.h_addrs_dev, 2 * list_bytes));
    if (fresh_list && !job.h_earlier) {   // (h_earlier: reserved last)
        HIP_TRY(c, pinned_alloc(c, &job.h_fresh, &job.h_fresh_dev, list_bytes));
        HIP_TRY(c, dev_alloc(c, &job.d_fresh_seen, kBitmapAllocWords * sizeof(uint32_t)));   // (also the `earlier` set of a scored shard)
        HIP_TRY(c, pinned_alloc(c, &job.h_earlier, &job.h_earlier_dev, list_bytes));
    }
    return undo.keep = true, ADSB_OK;
}

// Receivers scored on the device (adsb_set_receiver_scoring): per pass in flight a device copy of the map with its pinned
// staging, a keyed first-adder table the size of the slot's plain one, the keyed slot of every hit, and the receiver of
// every addition in mapped host memory; per context two keyed sets of 8 << rx_set_lg_for(n_receivers) bytes.  Reserved the
// first time the mode is on together with receivers, in a context that scores on the device at all; the sets are
// re-made when the number of receivers changes.  Nothing may be in flight.
uint32_t rx_set_lg_for(uint32_t n_receivers)
{
    uint32_t lg = kRxSetLgMin;   // 2 x 4096 slots for one receiver
    while (lg < kRxSetLgMax && (1ull << lg) < 2ull * IcaoFilter::kSize * std::max(1u, n_receivers)) lg++;
    return lg;
}

int ensure_rx_scoring(adsb_ctx *c)
{
    if (!c->score.si || !c->n_receivers) return ADSB_OK;
    const size_t hsize = (size_t)c->score.hash_mask + 1, map_bytes = up256(c->max_chunks * sizeof(uint32_t)),
                 per_slot = map_bytes + up256((size_t)c->score.cap * sizeof(uint32_t));
    const uint32_t want_lg = rx_set_lg_for(c->n_receivers);
    const bool new_slots = !c->d_rx_failed;   // (reserved last of the slots' part)
    const bool new_sets = !c->rx_set[1] || want_lg != c->rx_set_alloc_lg;   // (absent, or sized for another number of receivers)
    if (new_sets) {
        for (auto &st : c->rx_set) release(c, &st);
        c->rx_set_alloc_lg = 0;
    }
    Rollback undo{c->mem, c->mem.mark(), false};
    if (new_slots) {
        HIP_TRY(c, pinned_alloc(c, &c->h_rx_block, &c->h_rx_block_dev, per_slot * (size_t)c->n_slots));
        for (int si = 0; si < c->n_slots; si++) {
            Slot &sl = c->slot[si];
            HIP_TRY(c, dev_alloc(c, &sl.d_rx_map, c->max_chunks * sizeof(uint32_t)));
            HIP_TRY(c, dev_alloc(c, &sl.d_rx_slot, (size_t)c->score.cap * sizeof(uint32_t)));
            HIP_TRY(c, dev_alloc(c, &sl.d_rx_first, hsize * sizeof(unsigned long long)));
            HIP_TRY(c, hipMemset(sl.d_rx_first, 0xFF, hsize * sizeof(unsigned long long)));
        }
        HIP_TRY(c, dev_alloc(c, &c->d_rx_failed, sizeof(uint32_t)));
    }
    if (new_sets)
        for (auto &st : c->rx_set) HIP_TRY(c, dev_alloc(c, &st, sizeof(unsigned long long) << want_lg));
    undo.keep = true;
    uint32_t first_lg = 0;
    while (((size_t)1 << first_lg) < hsize) first_lg++;
    for (int si = 0; new_slots && si < c->n_slots; si++) {   // (the views, now that nothing can fail)
        Slot &sl = c->slot[si];
        sl.h_rx_map = reinterpret_cast<uint32_t *>(c->h_rx_block + per_slot * (size_t)si);
        sl.h_add_rx = reinterpret_cast<uint32_t *>(c->h_rx_block + per_slot * (size_t)si + map_bytes);
        sl.h_add_rx_dev = reinterpret_cast<uint32_t *>(c->h_rx_block_dev + per_slot * (size_t)si + map_bytes);
        sl.rx = RxScoreDev{};
        sl.rx.rx_map = sl.d_rx_map;
        sl.rx.first = sl.d_rx_first;
        sl.rx.first_lg = first_lg;
        sl.rx.rx_slot = sl.d_rx_slot;
        sl.rx.out_add_rx = sl.h_add_rx_dev;
    }
    if (new_sets) c->rx_set_alloc_lg = want_lg, c->cur_rx_set = 0;
    c->rx_set_valid = false;   // (the next scored pass fills them)
    return ADSB_OK;
}


}  // namespace host
}  // namespace adsb

extern "C" {

void adsb_destroy(adsb_ctx *c)
{
    if (!c) return;
    print_host_times(c);
    DeviceGuard on_device(c->device);
    // nothing the context put on a stream may still be running when its memory goes (shared streams: other contexts'
    // work on them is waited for too)
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    for (hipStream_t q : c->scan_stream)
        if (q) (void)hipStreamSynchronize(q);
    for (hipStream_t q : {c->tail_stream, c->score_stream})
        if (q) (void)hipStreamSynchronize(q);
    if (c->d_timeline) {   // (blocking copies out of it: the streams are idle)
        if (tuning_env("ADSB_TIMELINE") && std::atoi(tuning_env("ADSB_TIMELINE")) == 3) dump_onelaunch_timeline(c);
        else if (c->debug_stop == 100) dump_scan_phases(c);
        else dump_scan_stamps(c);
    }
    c->mem.release_all();
    for (const auto &r : c->host_ranges) (void)hipHostUnregister(r.base);
    if (c->private_streams) {
        for (hipStream_t q : {c->own_stream, c->tail_stream, c->score_stream})
            if (q) (void)hipStreamDestroy(q);
        for (hipStream_t q : c->scan_stream)
            if (q) (void)hipStreamDestroy(q);
    } else if (c->own_stream) {
        // the scan / tail / score streams are the device's (shared, never destroyed); the context's own goes back
        std::lock_guard<std::mutex> lk(g_streams_mu);
        for (DeviceStreams *d : g_device_streams)
            if (d->device == c->device) d->free_own.push_back(c->own_stream);
    }
    delete c;
}

int adsb_set_stream(adsb_ctx *c, void *hip_stream)
try {
    if (!c) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_set_profiling(adsb_ctx *c, int enabled)
try {
    if (!c) return ADSB_ERR_INVALID;
    // (the level decides whether a pass of a few buffers is one launch or three, and the cross-stream edges of a
    // pass are worked out from what the passes in flight are: like the other settings, only between passes)
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    c->profiling = enabled < 0 ? 0 : (enabled > 2 ? 2 : enabled);
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_set_carry_over(adsb_ctx *c, int enabled)
try {
    if (!c) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    // (the lead-in of a buffer would have to be the end of ITS receiver's previous buffer: adsb_set_receivers)
    if (enabled && c->n_receivers) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(c);
    c->carry_over = enabled != 0;
    // the stream starts here: nothing precedes the next call
    for (int si = 0; si < c->n_slots; si++)
        HIP_TRY(c, hipMemsetAsync(c->slot[si].d_carry, 0, kCarrySamples * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_carry_next, 0, kCarrySamples * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_set_error_correction(adsb_ctx *c, int mode)
try {
    if (!c || (mode != ADSB_FIX_NONE && mode != ADSB_FIX_1BIT && mode != ADSB_FIX_2BIT)) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    // (the one copy of the mode: the host replay scores with c->crc, and every pass built after this takes
    // ScanParams::fix from it)
    c->crc.set_fix(mode);
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_get_error_correction(const adsb_ctx *c) { return c ? c->crc.fix : ADSB_ERR_INVALID; }

int adsb_set_signal_stats(adsb_ctx *c, int enabled)
try {
    if (!c) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    if (enabled) {
        ADSB_ON_DEVICE(c);
        if (int rc = ensure_signal_stats(c)) return rc;
    }
    c->signal_stats = enabled != 0;
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_get_signal_stats(const adsb_ctx *c) { return c ? (c->signal_stats ? 1 : 0) : ADSB_ERR_INVALID; }
uint64_t adsb_selftest_signal_launches(const adsb_ctx *c) { return c ? c->sig_launches : 0; }

int adsb_fetch_signal_stats(adsb_ctx *c, adsb_signal_stats *out, size_t cap, size_t *n_out)
try {
    if (!c || (!out && cap)) return ADSB_ERR_INVALID;
    const size_t n = std::min(cap, c->sig_out.size());
    if (n) std::memcpy(out, c->sig_out.data(), n * sizeof(adsb_signal_stats));
    if (n_out) *n_out = c->sig_out.size();
    return c->sig_out.size() > cap ? ADSB_ERR_CAPACITY : ADSB_OK;
} ADSB_ABI_CATCH

int adsb_set_u8_table(adsb_ctx *c, const int16_t *table256)
try {
    if (!c) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    ADSB_ON_DEVICE(c);
    int16_t t[256];
    if (table256) std::memcpy(t, table256, sizeof t);
    else soapy_u8_table(t);
    // (nothing is in flight: every pass that read the old table has been collected)
    HIP_TRY(c, hipMemcpy(c->d_u8_table, t, sizeof t, hipMemcpyHostToDevice));
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_selftest_u8_table(adsb_ctx *c, int16_t *out256)
try {
    if (!out256) return ADSB_ERR_INVALID;
    if (!c) {
        soapy_u8_table(out256);
        return ADSB_OK;
    }
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    ADSB_ON_DEVICE(c);
    HIP_TRY(c, hipMemcpy(out256, c->d_u8_table, 256 * sizeof(int16_t), hipMemcpyDeviceToHost));
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_icao_flush(adsb_ctx *c)
{
    if (!c) return ADSB_ERR_INVALID;
    // Takes effect for everything submitted after this call: the next pass's reset kernel
    // clears the device bitmap (stream-ordered), and the host filter is flushed when that
    // pass is collected, after the passes before it have been replayed.
    c->flush_pending = true;
    return ADSB_OK;
}

// ---- many receivers, one pass (include/adsb_hip.h) ----
int adsb_set_receivers(adsb_ctx *c, uint32_t n_receivers)
try {
    if (!c || n_receivers > ADSB_MAX_RECEIVERS || (n_receivers && c->carry_over)) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    if (n_receivers == c->n_receivers) return ADSB_OK;
    // everything that can fail first: the filters of receivers 1 .. n - 1 (16 KB each) and, per pass in flight, room
    // for the largest map, so that no submit allocates
    std::vector<IcaoFilter> filters(n_receivers > 1 ? n_receivers - 1 : 0);
    std::vector<IcaoFilter *> filter_of(n_receivers);
    for (uint32_t r = 0; r < n_receivers; r++) filter_of[r] = r ? &filters[r - 1] : &c->filter;
    for (int si = 0; si < c->n_slots; si++) {
        c->slot[si].rx_map.reserve(n_receivers ? c->max_chunks : 0);
        c->slot[si].rx_map.clear();
        c->slot[si].rx_flush.clear();
    }
    c->rx_flush_next.clear();
    c->rx_filters.swap(filters);   // (the vector's elements stay where they are: filter_of points at them)
    c->rx_filter_of.swap(filter_of);
    c->n_receivers = n_receivers;
    // every receiver starts from an empty filter, as after adsb_icao_flush: the host's filters now (nothing is in
    // flight), the device's superset with the next pass; and the device's own copy of the one filter is rebuilt from
    // the host's before a pass is scored on the device again
    c->filter.flush();
    c->flush_pending = true;
    c->score_epoch++;
    c->exact_valid = false;
    c->rx_set_valid = c->rx_set_full = c->rx_held_valid = false;
    if (c->rx_scoring) {   // the keyed sets are sized from the number of receivers
        ADSB_ON_DEVICE(c);
        if (int rc = ensure_rx_scoring(c)) {
            // (both modes on, adsb_set_receiver_carry_scoring: the seams' storage is sized by the number of receivers too and
            // must not stay at the old one -- re-sized all the same; without keyed sets the passes are the host's)
            if (c->rx_carry && c->seam_receivers_changed) (void)c->seam_receivers_changed(c);
            return rc;
        }
    }
    if (c->rx_carry && c->seam_receivers_changed) {   // receiver seams: every stream restarts; n = 0 turns the mode off
        ADSB_ON_DEVICE(c);
        if (int rc = c->seam_receivers_changed(c)) return rc;
    }
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_get_receivers(const adsb_ctx *c) { return c ? (int)c->n_receivers : ADSB_ERR_INVALID; }

int adsb_icao_flush_receiver(adsb_ctx *c, uint32_t receiver)
try {
    if (!c || receiver >= c->n_receivers) return ADSB_ERR_INVALID;
    // Host only: the device's superset keeps the receiver's addresses (it stays a superset of every filter).  With
    // nothing left to replay the filter is emptied here; otherwise when the next pass submitted is collected, in front
    // of its replay, behind the replays of the passes in flight now.
    if (c->submitted == c->collected) {
        c->rx_filter_of[receiver]->flush();
        if (receiver < c->rx_held.size()) c->rx_held[receiver] = 0;
    } else {
        c->rx_flush_next.push_back(receiver);
    }
    // (scoring on the device: the keyed set cannot forget one receiver -- the next scored pass drains and rebuilds it)
    c->rx_set_valid = false;
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_receiver_filter_table(const adsb_ctx *c, uint32_t receiver, uint32_t *out4096)
try {
    if (!c || !out4096 || receiver >= c->n_receivers) return ADSB_ERR_INVALID;
    if (c->submitted != c->collected) return ADSB_ERR_BUSY;
    c->rx_filter_of[receiver]->store(out4096);
    // (flushes that wait for the next pass have emptied it as far as the caller is concerned)
    bool flushed = c->flush_pending;
    for (uint32_t r : c->rx_flush_next) flushed = flushed || r == receiver;
    if (flushed) std::memset(out4096, 0, IcaoFilter::kSize * sizeof(uint32_t));
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_selftest_rx_tune(adsb_ctx *c, uint32_t parallel_min)
{
    if (!c) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
    c->rx_parallel_min = parallel_min ? parallel_min : kRxParallelReplayMin;
    return ADSB_OK;
}

int adsb_selftest_rx_counters(const adsb_ctx *c, uint64_t *out4)
{
    if (!c || !out4) return ADSB_ERR_INVALID;
    out4[0] = c->rx_passes, out4[1] = c->rx_pooled, out4[2] = c->rx_reseeds, out4[3] = 0;
    return ADSB_OK;
}

// ---- receivers scored on the device (include/adsb_hip.h) ----
int adsb_set_receiver_scoring(adsb_ctx *c, int enabled)
try {
    if (!c) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    // (adsb_set_receiver_carry_scoring holds both modes on: the value in effect is fine, a change is not)
    if (c->rx_carry_scoring) return enabled ? ADSB_OK : ADSB_ERR_INVALID;
    if (enabled && c->rx_carry) return ADSB_ERR_INVALID;   // (seam trials are scored by the host: adsb_set_receiver_carry)
    if (enabled && !c->rx_scoring) {
        ADSB_ON_DEVICE(c);
        c->rx_scoring = true;   // (remembered whatever comes of it: adsb_set_receivers reserves what is missing)
        if (int rc = ensure_rx_scoring(c)) {
            c->rx_scoring = false;
            return rc;
        }
    }
    c->rx_scoring = enabled != 0;
    // either way the passes in flight are none, and the next scored pass of either kind rebuilds what it scores against
    c->rx_set_valid = false;
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_get_receiver_scoring(const adsb_ctx *c) { return c ? (c->rx_scoring ? 1 : 0) : ADSB_ERR_INVALID; }

int adsb_selftest_rx_score_counters(const adsb_ctx *c, uint64_t *out4)
{
    if (!c || !out4) return ADSB_ERR_INVALID;
    out4[0] = c->rx_scored_taken, out4[1] = c->rx_scored_refused, out4[2] = c->rx_set_rebuilds, out4[3] = c->rx_no_room;
    return ADSB_OK;
}

int adsb_selftest_rx_score_tune(adsb_ctx *c, uint32_t set_lg, uint32_t probe_max)
{
    if (!c || (set_lg && (set_lg < 4 || set_lg > kRxSetLgMax)) || probe_max > 4096) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
    c->rx_tune_lg = set_lg;
    c->rx_tune_probe = probe_max;
    c->rx_set_valid = c->rx_set_full = false;   // (the sets are re-made with the new geometry before they are used again)
    return ADSB_OK;
}

uint32_t adsb_rx_set_home(uint64_t key, uint32_t set_lg) { return set_lg >= 1 && set_lg <= 32 ? rx_set_home(key, set_lg) : 0u; }

int adsb_selftest_rx_set_lookup(adsb_ctx *c, const uint64_t *keys, size_t n_keys, const uint64_t *queries, size_t n_q, uint32_t *out)
try {
    if (!c || !out || (!keys && n_keys) || (!queries && n_q) || n_keys > (1u << 24) || n_q > (1u << 24)) return ADSB_ERR_INVALID;
    for (size_t i = 0; i < n_keys; i++)
        if (keys[i] == ~0ull) return ADSB_ERR_INVALID;   // (the empty slot's value: no (receiver, value) pair makes it)
    ADSB_ON_DEVICE(c);
    // a scratch set with the geometry the context's own sets have now (the tuned one, or the default for its receivers)
    const uint32_t dflt = rx_set_lg_for(c->n_receivers);
    const uint32_t lg = c->rx_tune_lg ? std::min(c->rx_tune_lg, dflt) : dflt, probe_max = c->rx_probe_max();
    const size_t set_bytes = sizeof(unsigned long long) << lg, in_bytes = (n_keys + n_q) * sizeof(unsigned long long);
    ScratchRegistry scratch;   // (its release waits for whatever an early return leaves on the stream)
    char *d = nullptr;
    const size_t o_in = set_bytes, o_out = o_in + up256(in_bytes), total = o_out + (n_q + 1) * sizeof(uint32_t);
    HIP_TRY(c, scratch.add(Registry::kDevice, (void **)&d, total));
    unsigned long long *d_set = reinterpret_cast<unsigned long long *>(d), *d_in = reinterpret_cast<unsigned long long *>(d + o_in);
    uint32_t *d_out = reinterpret_cast<uint32_t *>(d + o_out);
    c->own_stream_dirty = true;
    HIP_TRY(c, hipMemsetAsync(d_set, 0xFF, set_bytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_out, 0, (n_q + 1) * sizeof(uint32_t), c->stream));
    if (n_keys) HIP_TRY(c, hipMemcpyAsync(d_in, keys, n_keys * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    if (n_q) HIP_TRY(c, hipMemcpyAsync(d_in + n_keys, queries, n_q * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    if (int e = launch_rx_set_fill(d_in, (uint32_t)n_keys, d_set, lg, probe_max, d_out + n_q, c->stream)) return fail(c, (hipError_t)e, "launch_rx_set_fill");
    if (int e = launch_rx_set_lookup(d_in + n_keys, (uint32_t)n_q, d_set, lg, probe_max, d_out, c->stream)) return fail(c, (hipError_t)e, "launch_rx_set_lookup");
    HIP_TRY(c, hipMemcpyAsync(out, d_out, (n_q + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return ADSB_OK;
} ADSB_ABI_CATCH

uint64_t adsb_host_sorts(const adsb_ctx *c) { return c ? c->host_sorts : 0; }
uint64_t adsb_host_replays(const adsb_ctx *c) { return c ? c->host_replays : 0; }
uint64_t adsb_host_rematches(const adsb_ctx *c) { return c ? c->rematches : 0; }
int adsb_max_in_flight(const adsb_ctx *c) { return c ? c->n_slots : 0; }

int adsb_get_stats(const adsb_ctx *c, adsb_stats *out)
{
    if (!c || !out) return ADSB_ERR_INVALID;
    *out = c->stats;
    return ADSB_OK;
}

const char *adsb_last_error(const adsb_ctx *c) { return c ? c->last_error.c_str() : ""; }

const char *adsb_version(void) { return "adsb_hip 0.23 gfx950 scan=v10-sparse-folded tail=v8-sparse-lean multi=v3-bounded-waits streams=v2-own-queues stats=v1 rxscore=v1"; }

}  // extern "C"
