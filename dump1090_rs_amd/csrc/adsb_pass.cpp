// adsb_pass.cpp -- one device pass: what is enqueued on which stream (every cross-stream event edge is here;
// docs/HISTORY.md section 5b is the table to review it against), submit, and the blocking entry points
// (reference: src/utils.rs:43 to_mag, src/demod_2400.rs:115 demodulate2400, dump1090_rs/src/main.rs:166-167).
#include "adsb_ctx.h"

using namespace adsb::host;

namespace adsb {
namespace host {

// `sl` with the worst-case lists in place of its own: what a one-buffer fallback pass runs on
// (same counters, AP list, summary, events and carry as the pass it redoes).
int fallback_slot(adsb_ctx *c, const Slot &sl, Slot &tmp)
{
    if (int rc = ensure_fallback(c)) return rc;
    tmp = sl;
    tmp.d_hits = c->fb.d_hits;
    tmp.h_rec = c->fb.h_rec;
    tmp.h_rec_dev = c->fb.h_rec_dev;
    tmp.hits_cap = kWorstPerChunk;
    return ADSB_OK;
}

int put_behind(adsb_ctx *c, hipStream_t waiter, hipStream_t ahead)
{
    if (!ahead || ahead == waiter) return ADSB_OK;
    HIP_TRY(c, hipEventRecord(c->lazy_ev, ahead));
    HIP_TRY(c, hipStreamWaitEvent(waiter, c->lazy_ev, 0));
    return ADSB_OK;
}

// `waiter` waits until `other`'s pass is through matching (its records kernel has finished): the event
// behind a three-launch pass, or -- a one-launch pass records none -- an event put on its stream now.
int wait_for_tail_of(adsb_ctx *c, hipStream_t waiter, Slot &other)
{
    if (other.fused) return put_behind(c, waiter, other.tail_q);
    HIP_TRY(c, hipStreamWaitEvent(waiter, other.recorded, 0));
    return ADSB_OK;
}

int order_behind_fused(adsb_ctx *c, Slot &sl, hipStream_t waiter)
{
    if (int rc = put_behind(c, waiter, sl.fused_q)) return rc;
    sl.fused_q = nullptr;
    return ADSB_OK;
}

// The tuning knobs of a pass (tuning builds only: adsb_device.h, tuning_env), each read once, here.
static bool knob_no_fuse() { static const bool v = tuning_env("ADSB_NO_FUSE") != nullptr; return v; }
static int knob_fused_streams() { static const int v = tuning_env("ADSB_FUSED_STREAMS") ? std::atoi(tuning_env("ADSB_FUSED_STREAMS")) : kScanStreams; return v; }
static bool knob_one_scan_stream() { static const bool v = tuning_env("ADSB_ONE_SCAN_STREAM") != nullptr; return v; }
static bool knob_no_hit_fields() { static const bool v = tuning_env("ADSB_NO_HIT_FIELDS") != nullptr; return v; }
static bool knob_ext_events() { static const bool v = !tuning_env("ADSB_NO_EXT_EVENTS"); return v; }
static bool knob_no_trickle() { static const bool v = tuning_env("ADSB_NO_TRICKLE") != nullptr; return v; }
static bool knob_skip_match() { static const bool v = tuning_env("ADSB_SKIP_MATCH") != nullptr; return v; }   // measurement aid: wrong results

// Whether a plain pass of n_chunks buffers submitted now goes out as one launch.
bool one_launch_pass(const adsb_ctx *c, uint32_t n_chunks)
{
    return !knob_no_fuse() && c->profiling <= 1 && n_chunks <= (uint32_t)kInlineTailChunks;
}

// The stream rule: consecutive pipelined passes rotate over the scan streams (three-launch passes over the first
// two, one-launch passes over up to four), unless something orders consecutive passes (the carry hand-off) or the
// pass is a one-off (a redo, the reference-shaped kernel, caller-supplied magnitudes: not `plain_iq`).
// (a slot's passes of one kind always land on the same stream: the slot count is a multiple of both periods)
static int scan_stream_index(const adsb_ctx *c, bool plain_iq, bool carry, bool one_launch, bool redo)
{
    if (!plain_iq || carry || redo || knob_one_scan_stream()) return 0;
    const int period = one_launch ? std::max(1, std::min(knob_fused_streams(), c->n_scan_streams)) : 2;
    return (int)(c->submitted % (uint64_t)period);
}

// The scan stream the next plain IQ pass of n_chunks buffers will run on.
hipStream_t next_scan_stream(const adsb_ctx *c, uint32_t n_chunks)
{
    return c->scan_stream[scan_stream_index(c, true, ordered_passes(c), one_launch_pass(c, n_chunks), false)];
}

void pass_params(adsb_ctx *c, const Slot &sl, ScanParams &p, uint32_t **retired, uint32_t *clear_next)
{
    *retired = nullptr;
    *clear_next = 0;
    p.bitmap_lg = c->bitmap_lg;
    if (c->flush_pending) {  // icao_flush: retire the bitmap in use, continue on the next one
        // Full bitmaps (2 MiB): the next one IS clean, and the records kernel of this pass (of a shard's second phase)
        // cleans the retired one behind the passes still matching against it (edge 1).  Folded ones (64 KB, contexts
        // for passes of a few buffers): the retired one is left as it is and the NEXT one is cleared before this pass
        // first touches it -- in its own launch (k_scan_fast<FUSED>: bitmap_fresh) or with a reset launch in front of
        // its scan.  Whoever used that bitmap has been collected (one bitmap more than passes in flight), so the pass
        // waits for nobody: an icao_flush before every pass, the reference's own benchmark shape
        // (benches/demod_benchmark.rs:9), used to cost a pipelined one-buffer pass 99 us instead of 5.7
        // (profiles/r4_v18_hosttime_ring.txt).
        if (c->bitmap_lg == kFullBitmapLg) *retired = c->d_bitmap[c->cur_bitmap];
        else *clear_next = 1;
        c->cur_bitmap = (c->cur_bitmap + 1) % c->n_bitmaps;
    }
    p.bitmap = c->d_bitmap[c->cur_bitmap];
    p.hits = sl.d_hits;
    p.hits_cap = sl.hits_cap;
    p.ap = sl.d_ap;
    p.ap_cap = c->ap_cap;
    p.seg_cap = c->seg_cap;
    p.tables = c->d_tables;
    p.fix = (uint32_t)c->crc.fix;
    p.ctr = sl.d_ctr;
    p.summary = sl.h_sum_dev;
}

void wire_score(const Slot &sl, ScanParams &p, uint32_t *exact, uint32_t *exact_retired)
{
    p.score = sl.score;
    p.score.exact = exact;
    p.score.exact_retired = exact_retired;
    p.score.out_msgs = sl.h_msgs_dev;
    p.score.out_adds = sl.h_adds_dev;
    p.score.summary = sl.h_ssum_dev;
}

uint32_t next_seq(adsb_ctx *c)
{
    const uint32_t s = c->next_seq++;
    if (c->next_seq == 0) c->next_seq = 1;
    return s;
}

void stamp_seq(adsb_ctx *c, Slot &sl, ScanParams &p, bool scored)
{
    sl.seq = next_seq(c);
    sl.h_sum->seq = 0;  // the records kernel overwrites it, last, with sl.seq
    p.seq = sl.seq;
    if (scored) {
        p.score.seq = sl.seq;
        sl.h_ssum->seq = 0;
    }
}

// ---- one device pass, step by step (docs/HISTORY.md section 5b: the table of the cross-stream edges they name) ----
// What plan_pass decides about a pass before anything is filled in or enqueued.
struct PassPlan {
    bool from_mag = false, fast = false;    // caller-supplied magnitudes / IQ through the fast scan (not the reference-shaped one)
    bool ordered = false, scored = false;   // the device hands the hits over in (buffer, j, try_phase) order / and scored
    bool fused = false, classic = false;    // one launch (k_scan_fast<.., FUSED>) / event records around the scan launch
    bool inline_tail = false;               // the tail stays on the scan stream
    int prof = 0, si = 0;                   // the profiling level of the pass; its scan stream, as an index and as it is
    hipStream_t ss = nullptr;
};

// Step 1 -- what kind of pass this is.  Places no edge; a device-scored pass behind one the host scored itself
// drains and rebuilds first (row 7 of the table).
static int plan_pass(adsb_ctx *c, const Slot &sl, SrcFormat fmt, uint32_t n_chunks, const PassOptions &opt, PassPlan &pl)
{
    pl.from_mag = fmt == SrcFormat::kMag;
    pl.fast = !pl.from_mag && !opt.force_simple;
    // Passes of many buffers of a dense stream hand their hits over in (buffer, j, try_phase) order and scored; a small
    // pass is all launch overhead and a sparse one leaves a few hundred records that the host sorts and scores in no
    // time; the worst-case lists of the fallback are the host's too.
    pl.ordered = !opt.force_simple && n_chunks > kInlineTailChunks && sl.hits_cap == c->hits_cap && c->dense_mode;
    // (in every error-correction mode: k_score / k_emit score and repair a fix pass's DF17/18 trials themselves)
    // (with receivers on only where adsb_set_receiver_scoring asked for it: k_score holds ONE filter, such a pass goes
    // through the keyed kernels of adsb_score_rx.hip; otherwise its replay is the host's, buffer by buffer)
    const bool rx = c->n_receivers != 0;
    if (rx && c->flush_pending) c->rx_set_full = false;   // (every filter starts empty again: so can the keyed set)
    // (receiver seams: only with the device-side merge's storage in hand, adsb_set_receiver_carry_scoring -- a seam pass
    // scored without it would lack its seam records)
    const bool score_on_device = pl.ordered && c->score.si && (!rx || (c->rx_scoring && c->rx_set[0] && !c->rx_set_full)) &&
                                 (!c->rx_carry || c->d_merge_block);
    if (score_on_device && rx) {
        if (!c->rx_set_valid) {
            // the keyed set can only be rebuilt from the host's filters once every pass in flight has been replayed:
            // finish them now (their results wait for adsb_collect).  The receiver flushes recorded against this pass
            // are what made the set invalid, or come behind whatever did: every earlier pass has been replayed by
            // then, so they are applied to the host's filters here, in front of the rebuild.
            if (int rc = park_pending(c)) return rc;
            flush_receivers(c, c->rx_flush_next);
            if (int rc = rebuild_rx_set(c)) return rc;
        }
        pl.scored = c->rx_set_valid;
    } else {
        if (score_on_device && !c->exact_valid) {
            // the device's copy of the filter can only be rebuilt from the host's once every pass in
            // flight has been replayed: finish them now (their results wait for adsb_collect)
            if (int rc = park_pending(c)) return rc;
            if (int rc = resync_exact(c)) return rc;
        }
        pl.scored = score_on_device && c->exact_valid;
    }
    pl.prof = c->profiling;   // 1: the scan launch stamps its own begin / end; 2: classic event records between all kernels
    // A pass of a few buffers is all launch overhead and event traffic: it goes out as ONE launch whose last workgroup
    // matches, builds the records and publishes the summary, with no event behind it.  (Level 2 wants the kernels apart.)
    pl.fused = !opt.force_simple && !opt.no_fuse && one_launch_pass(c, n_chunks);
    pl.classic = !pl.fused && (pl.prof > 1 || (pl.prof == 1 && (!pl.fast || !knob_ext_events())));
    pl.si = scan_stream_index(c, pl.fast, (c->carry_over && !pl.from_mag && sl.d_carry) || c->rx_carry, pl.fused, opt.redo);
    pl.ss = c->scan_stream[pl.si];
    // A small pass is all launch overhead: its tail stays on its scan stream too (the scan streams still let
    // consecutive passes overlap), which saves the cross-stream hand-off.
    pl.inline_tail = opt.inline_tail || n_chunks <= kInlineTailChunks;
    return ADSB_OK;
}

// Step 2 -- the pass's ScanParams and the slot's bookkeeping; consumes a pending icao_flush.  Places no edge.
static void fill_pass(adsb_ctx *c, Slot &sl, ScanParams &p, const void *d_src, SrcFormat fmt, uint64_t n_samples,
                      uint32_t n_chunks, const PassOptions &opt, const PassPlan &pl)
{
    p.src = d_src;
    p.n_samples = n_samples;
    p.n_chunks = n_chunks;
    pass_params(c, sl, p, &p.clean_bitmap, &p.bitmap_fresh);
    p.dap = c->fb.d_dap;  // only the reference-shaped kernel writes it (force_simple: fallback_slot() came first)
    p.dap_cap = c->fb.d_dap ? kWorstPerChunk : 0;
    p.stagger_ticks = c->stagger_ticks;
    p.debug_stop = c->debug_stop;
    p.timeline = c->d_timeline;
    p.carry = c->carry_over && !pl.from_mag ? sl.d_carry : nullptr;
    p.u8_table = fmt == SrcFormat::kCu8 ? c->d_u8_table : nullptr;
    p.lead_from_src = opt.lead_from_src ? 1u : 0u;
    p.order_cnt = pl.ordered ? sl.d_order_cnt : nullptr;
    p.order_base = pl.ordered ? sl.d_order_base : nullptr;
    p.order_tmp = pl.ordered ? sl.d_order_tmp : nullptr;
    // the scan hands the bit fields of its self-validating hits to the record builder: where the record builder's
    // instructions matter (dense streams: it shares the vector pipes with the next scan) and in one-launch passes; a
    // sparse stream's scan stays the lean instantiation (and the reference-shaped kernel, the fallback's, fills none)
    p.hit_fields = pl.fused || (pl.ordered && !knob_no_hit_fields()) ? sl.d_hit_fields : nullptr;
    sl.device_scored = pl.scored;
    sl.rx_scored = pl.scored && c->n_receivers;
    if (sl.rx_scored) {
        // the plain exact bitmap is not this pass's business (no rotation, nothing retired); the keyed set is
        unsigned long long *set_retired = nullptr;
        if (c->flush_pending) {  // icao_flush: this pass starts from the empty keyed set
            set_retired = c->rx_set[c->cur_rx_set];
            c->cur_rx_set ^= 1;
        }
        wire_score(sl, p, c->exact_bm[c->cur_exact], nullptr);
        sl.rx.set = c->rx_set[c->cur_rx_set];
        sl.rx.set_lg = c->rx_set_lg();
        sl.rx.probe_max = c->rx_probe_max();
        sl.rx.set_retired = set_retired;
        sl.rx.retired_lg = c->rx_set_alloc_lg;   // (the whole allocation, whatever geometry the passes before used)
        sl.score_epoch = c->score_epoch;
    } else if (pl.scored) {
        uint32_t *exact_retired = nullptr;
        if (c->flush_pending) {  // icao_flush: this pass starts from the clean exact bitmap
            exact_retired = c->exact_bm[c->cur_exact];
            c->cur_exact ^= 1;
        }
        wire_score(sl, p, c->exact_bm[c->cur_exact], exact_retired);
        sl.score_epoch = c->score_epoch;
    }
    p.fused_rec = pl.fused ? sl.h_rec_dev : nullptr;
    p.order_polls = c->order_polls;
    p.src_ready = pl.fused && !pl.from_mag ? c->next_src_ready : nullptr;
    c->next_src_ready = nullptr;
    p.src_host = pl.fused && !pl.from_mag && c->next_src_host && !knob_no_trickle() ? 1u : 0u;
    c->next_src_host = false;
    sl.src = d_src;
    sl.fmt = fmt;
    sl.n_samples = n_samples;
    sl.n_chunks = n_chunks;
    sl.flush_before = c->flush_pending;
    c->flush_pending = false;
    sl.profiled = pl.prof;
    sl.fused = pl.fused;
    sl.unsynced_from = 0;
    stamp_seq(c, sl, p, sl.device_scored);
    // A pass collect_oldest runs again keeps its number -- a fresh one per buffer would walk through the event ring
    // under the passes still in flight and move last_new_insert_seq ahead of them -- and times itself with its own pair.
    sl.redo = opt.redo;
    if (!sl.redo) sl.scan_seq = ++c->scan_counter;
    const hipEvent_t *ev = sl.redo ? c->redo_ev : c->scan_ev[sl.scan_seq % kScanEvRing];
    sl.ev[0] = ev[0], sl.ev[1] = ev[1];
    // (a one-launch pass times itself on the device's wall clock and reports it with its summary)
    const bool stamps = knob_ext_events() && pl.prof == 1 && pl.fast && !pl.fused;
    p.ev_start = stamps ? sl.ev[0] : nullptr;
    p.ev_stop = stamps ? sl.ev[1] : nullptr;
}

// Step 3 -- edge "in": the scan stream behind the pass's input, which is complete at `input_done` (the caller's
// event), already (input_ready_now: pinned memory the host has filled), or where `stream` stands now.
int order_behind_input(adsb_ctx *c, hipEvent_t input_done, int si, hipStream_t ss)
{
    if (input_done != input_ready_now()) {
        HT(c, HT_IN_READY);
        hipEvent_t ready = input_done;
        // No event at all when `stream` is the context's own and the library has put nothing on it that this pass could
        // depend on (own_stream_dirty: the copies of the host-pointer entry points): the record + wait pair is two thirds
        // of what a one-launch pass costs the submitting thread.  (hipStreamQuery is no substitute: on a stream that has
        // seen work it took ~25 us, measured.)  A caller's stream (adsb_set_stream) is always waited for.
        const bool nothing_to_wait_for = !ready && c->stream == c->own_stream && !c->own_stream_dirty;
        if (!ready && !nothing_to_wait_for) {
            ready = c->input_ready[si];
            HIP_TRY(c, hipEventRecord(ready, c->stream));
            c->own_stream_dirty = false;   // (what was on it is now behind this pass)
        }
        if (ready) HIP_TRY(c, hipStreamWaitEvent(ss, ready, 0));
    }
    // (a ring slot's copy was queued on next_scan_stream(), which is the rule plan_pass applied: the same stream for
    // the pass adsb_ring_submit announced.  A pass that is not that one -- a redo, a shard -- waits for the copy.)
    return put_behind(c, ss, c->input_on_stream);
}

// Step 4 -- the edges in front of the scan launch: 0, 1'' and, for a one-launch pass, 1, 2 and 3'.
// (1) A bitmap an icao_flush retired is cleared by this pass (its records kernel, or every workgroup of a one-launch
//     pass): not before the passes still in flight, whichever stream their tail is on, are through matching against
//     it.  A tail on this same in-order stream is behind us already.
// (2) The match must see every address bit the scans of this and of all earlier passes set.  Behind its own scan it
//     is in stream order or waits for `scanned` (2').  Behind the previous pass's scan it is in order when both
//     matches run on the tail stream; a match on its own scan stream waits for the previous scan explicitly when that
//     ran on another one.  (Scans before the previous one are behind this pass's or the previous pass's.)
// (3) One-launch passes record no event and do not wait for each other across the scan streams: a three-launch pass
//     that needs one behind it records an event on that stream now (enqueue_tail); a one-launch pass notes from which
//     pass on its match is unsynchronised (3': Slot::unsynced_from) and the host redoes it if one of those taught
//     the filter a new address.
static int edges_before_scan(adsb_ctx *c, Slot &sl, const ScanParams &p, const PassPlan &pl)
{
    hipStream_t ss = pl.ss;
    // (0) the slot's lists and counters: a one-launch pass that used them last on another stream may still
    //     be zeroing them (the host goes by its summary, which it writes just before)
    if (int rc = order_behind_fused(c, sl, ss)) return rc;
    sl.fused_q = pl.fused ? ss : nullptr;
    // (1'') folded bitmaps: a pass behind the one that opened the filter's epoch shares the bitmap that one clears
    bool behind_fresh = false;   // this launch has been ordered behind the pass that opened the epoch
    if (c->bitmap_lg != kFullBitmapLg) {
        const long my_slot = &sl - c->slot;   // (a fallback pass's temporary slot is none of the context's)
        if (p.bitmap_fresh) {   // this pass opens the filter's next epoch and clears its bitmap
            c->fresh_q = ss;
            c->fresh_seq = c->epoch_first_seq = sl.scan_seq;
            c->fresh_slot = my_slot >= 0 && my_slot < kSlots ? (int)my_slot : -1;
        } else if (c->fresh_q && c->fresh_q != ss && c->fresh_slot >= 0 && c->fresh_slot != my_slot) {
            const Slot &f = c->slot[c->fresh_slot];
            if (f.busy && f.scan_seq == c->fresh_seq) {   // still in flight: behind it (rare: the first passes after a flush)
                if (int rc = put_behind(c, ss, c->fresh_q)) return rc;
                behind_fresh = true;
            }
        }
    }
    if (pl.fused) {
        HT(c, HT_EV_SCANNED);
        // (1), one launch
        if (p.clean_bitmap)
            for (Slot &other : c->slot)
                if (&other != &sl && other.busy && other.tail_q != ss)
                    if (int rc = wait_for_tail_of(c, ss, other)) return rc;
        // (2), one launch
        bool other_stream_synced = false;
        if (c->prev_scan_stream && c->prev_scan_stream != ss && !c->prev_fused && c->prev_scanned) {
            HIP_TRY(c, hipStreamWaitEvent(ss, c->prev_scanned, 0));
            other_stream_synced = true;   // (in stream order behind it: every earlier pass on that stream)
        }
        // (3') every pass in flight whose scan is not in stream order before this launch: not on this stream, and not on
        // the stream of the three-launch pass just waited for -- that wait covers what ran on ITS stream only -- and that
        // belongs to the filter's current epoch: what a pass from before the latest icao_flush taught the filter is gone
        // when this pass is replayed (with a flush before every pass every pass used to be redone for its predecessor's sake)
        for (Slot &other : c->slot)
            if (&other != &sl && other.busy && other.scan_q != ss && other.scan_seq >= c->epoch_first_seq &&
                !(other_stream_synced && other.scan_q == c->prev_scan_stream) && !(behind_fresh && other.scan_seq == c->fresh_seq))
                sl.unsynced_from = sl.unsynced_from ? std::min(sl.unsynced_from, other.scan_seq) : other.scan_seq;
    }
    sl.scan_q = ss;
    return ADSB_OK;
}

// Step 5 -- the scan launch and what goes with it on the scan stream: the clear of a fresh folded bitmap, the
// classic event records, the carry hand-off (row 6: stream order on scan[0], no edge).
static int launch_scan_step(adsb_ctx *c, Slot &sl, ScanParams &p, SrcFormat fmt, const PassOptions &opt, const PassPlan &pl)
{
    hipStream_t ss = pl.ss;
    if (p.bitmap_fresh && !pl.fused) {
        // (three launches in a context of folded bitmaps -- level-2 profiling, a caller's MagnitudeBuffer that
        // overflowed -- : the clear as a launch of its own in front of the scan; the counters it also zeroes are zero)
        if (int e = launch_reset(sl.d_ctr, p.bitmap, p.bitmap_lg, ss)) return fail(c, (hipError_t)e, "launch_reset");
        p.bitmap_fresh = 0;
    }
    if (pl.classic) HIP_TRY(c, hipEventRecord(sl.ev[0], ss));
    const bool hand_carry_on = p.carry && !opt.redo;
    if (hand_carry_on)  // this pass's lead-in: where the previous submission ended
        HIP_TRY(c, hipMemcpyAsync(sl.d_carry, c->d_carry_next, kCarrySamples * sizeof(uint32_t),
                                  hipMemcpyDeviceToDevice, ss));
    {
        HT(c, HT_SCAN_LAUNCH);
        bool ran_sparse = false;
        if (int e = pl.fused ? launch_pass_fused(p, fmt, ss)
                             : (opt.force_simple ? launch_scan_simple(p, fmt, ss) : launch_scan(p, fmt, ss, c->sparse_scan, &ran_sparse)))
            return fail(c, (hipError_t)e, "launch_scan");
        if (ran_sparse) c->sparse_scans++;
    }
    if (pl.classic) HIP_TRY(c, hipEventRecord(sl.ev[1], ss));
    if (hand_carry_on) {
        // the next submission starts from the end of this one's input (taken now: the caller
        // may reuse the buffer as soon as this pass is collected)
        if (int e = launch_update_carry(sl.d_carry, p.src, p.n_samples, c->d_carry_next, ss, p.u8_table))
            return fail(c, (hipError_t)e, "launch_update_carry");
    }
    return ADSB_OK;
}

// Step 6 -- the tail of a three-launch pass: match, order, records, with the edges 1, 2, 2' and 3 in front of them
// and `recorded` behind them.
static int enqueue_tail(adsb_ctx *c, Slot &sl, const ScanParams &p, SrcFormat fmt, const PassPlan &pl)
{
    hipStream_t ss = pl.ss;
    // the tail runs on its own stream behind the scan: the next pass's scan does not wait for it (it works on the other
    // slot's lists and counters); a blocking call's and a small pass's stay on the scan stream (plan_pass)
    hipStream_t ts = pl.inline_tail ? ss : c->tail_stream;
    if (p.clean_bitmap && pl.fast) {
        // edge (1): the event behind the other passes' records kernels, not `done`, which device-scored
        // passes record later, on the score stream
        for (Slot &other : c->slot)
            if (&other != &sl && other.busy && other.tail_q != ts)
                if (int rc = wait_for_tail_of(c, ts, other)) return rc;
    }
    {
        HT(c, HT_EV_SCANNED);
        // edge (2'): behind its own scan
        HIP_TRY(c, hipEventRecord(sl.scanned, ss));
        if (!pl.inline_tail) HIP_TRY(c, hipStreamWaitEvent(ts, sl.scanned, 0));
        // edge (2): behind the previous pass's scan
        if (c->prev_scanned && !c->prev_fused && c->prev_scan_stream != ss && (pl.inline_tail || c->prev_inline))
            HIP_TRY(c, hipStreamWaitEvent(ts, c->prev_scanned, 0));
        // edge (3): one-launch passes in flight on a stream this match is not behind
        for (hipStream_t q : c->scan_stream) {
            if (!q || q == ts || (q == ss && !pl.inline_tail)) continue;   // (behind its own scan: behind everything on that stream)
            bool any = false;
            for (Slot &other : c->slot) any = any || (&other != &sl && other.busy && other.fused && other.tail_q == q);
            if (!any) continue;
            if (int rc = put_behind(c, ts, q)) return rc;
        }
    }
    c->prev_scanned = sl.scanned;
    c->prev_scan_stream = ss;
    c->prev_inline = pl.inline_tail;
    c->prev_fused = false;
    if (pl.prof > 1) HIP_TRY(c, hipEventRecord(sl.ev[2], ts));
    // a sparse stream's pass in a large context: the lean match and the small records grid (adsb_aux.hip)
    const bool sparse_fast = pl.fast && !pl.ordered && c->bitmap_lg == kFullBitmapLg;
    {
        HT(c, HT_MATCH_LAUNCH);
        if (!knob_skip_match())
            if (int e = launch_match(p, ts, sparse_fast)) return fail(c, (hipError_t)e, "launch_match");
        if (int e = launch_order_hits(p, ts)) return fail(c, (hipError_t)e, "launch_order_hits");
    }
    if (pl.prof > 1) HIP_TRY(c, hipEventRecord(sl.ev[3], ts));
    // the records kernel writes the records and the summary into the slot's mapped host
    // memory with write-through stores; `done` only has to say the kernel has drained
    {
        HT(c, HT_RECORDS_LAUNCH);
        if (int e = launch_records(p, fmt, sl.h_rec_dev, ts, sparse_fast)) return fail(c, (hipError_t)e, "launch_records");
    }
    sl.tail_q = ts;
    // (always: a later pass whose own tail runs on another stream -- a small one behind an icao_flush --
    // waits for this event before its records kernel clears the bitmap this pass matched against)
    {
        HT(c, HT_EV_DONE);
        HIP_TRY(c, hipEventRecord(sl.recorded, ts));
    }
    return ADSB_OK;
}

// Step 6b -- the pass's signal statistics (adsb_set_signal_stats), only when the mode is on: k_signal_stats over the
// pass's input, one record per buffer into the slot's part of the context's mapped block.  It obeys the stream rule the
// scan obeys -- it goes out on the scan stream plan_pass chose, in front of the scan launch, behind the same input edge
// and edge 0 (the slot's partials are the slot's lists' kin) -- and places no edge of its own: the scan, and behind it the
// tail or the one launch's last workgroup, which publish the pass's summary, are in stream order behind it, so the
// summary never lands before the records have.  A pass that is run again (overflow fallback, rematch) and the reference-
// shaped kernel's passes launch none: the records of the first enqueue stand, computed once.
static int enqueue_signal_stats(adsb_ctx *c, Slot &sl, const ScanParams &p, SrcFormat fmt, const PassOptions &opt, const PassPlan &pl)
{
    if (opt.redo) return ADSB_OK;   // (sl.sig_on stays what the pass's first enqueue made it)
    sl.sig_on = c->signal_stats && pl.fast && sl.h_sig != nullptr;
    if (!sl.sig_on) return ADSB_OK;
    SigParams sp{};
    sp.src = p.src;
    sp.n_samples = p.n_samples;
    sp.n_chunks = p.n_chunks;
    sp.wg_per_chunk = signal_stats_wg_per_chunk(p.n_chunks);
    sp.u8_table = p.u8_table;
    sp.partial = sl.d_sig_part;
    sp.ticket = sl.d_sig_ticket;
    sp.records = sl.h_sig_dev;
    // (what take_signal_records checks every 8-byte word of every record against: no word of a record is ever all ones,
    // so a piece of the slot's previous pass cannot pass for this one's)
    std::memset(sl.h_sig, 0xFF, (size_t)p.n_chunks * sizeof(adsb_signal_stats));
    if (int e = launch_signal_stats(sp, fmt, pl.ss)) return fail(c, (hipError_t)e, "launch_signal_stats");
    c->sig_launches++;
    return ADSB_OK;
}

// Step 7 -- scoring on the device (edge 4) and the completion event (edge 5).
static int enqueue_score(adsb_ctx *c, Slot &sl, const ScanParams &p, const PassPlan &pl)
{
    hipStream_t ts = sl.tail_q;
    if (sl.device_scored) {
        // Scoring runs on its own in-order stream behind this pass's records kernel, so that the next pass's match /
        // order / records (tail stream) overlap it: every kernel beside the persistent scan is latency, and one chain of
        // eight would be longer than the scan it hides behind.  The score stream's order is the filter's order:
        // k_score(i+1) reads the exact bitmap after k_emit(i) has committed pass i's additions to it.
        hipStream_t qs = c->score_stream;
        HIP_TRY(c, hipStreamWaitEvent(qs, sl.recorded, 0));   // edge (4)
        if (sl.rx_scored) {
            // a receivers pass: the map, out of its pinned staging, in stream order in front of the three keyed kernels
            // (the slot's previous pass read its copy earlier on this very stream)
            std::memcpy(sl.h_rx_map, sl.rx_map.data(), (size_t)p.n_chunks * sizeof(uint32_t));
            HIP_TRY(c, hipMemcpyAsync(sl.d_rx_map, sl.h_rx_map, (size_t)p.n_chunks * sizeof(uint32_t), hipMemcpyHostToDevice, qs));
            // receiver seams scored on the device: behind the pass's k_seam_match (edge 4s) the seam records are merged
            // into the ordered hits, and the keyed kernels take the merged arrays for the pass's (any other pass: pm = p)
            ScanParams pm;
            if (int rc = seam_merge(c, sl, p, &pm, qs)) return rc;
            if (int e = launch_score_rx(pm, sl.rx, qs)) return fail(c, (hipError_t)e, "launch_score_rx");
        } else if (int e = launch_score(p, qs)) return fail(c, (hipError_t)e, "launch_score");
        ts = qs;
    }
    if (pl.prof > 1) HIP_TRY(c, hipEventRecord(sl.ev[4], ts));
    {
        HT(c, HT_EV_DONE);
        HIP_TRY(c, hipEventRecord(sl.done, ts));   // edge (5)
    }
    return ADSB_OK;
}

// Enqueue one device pass over n_chunks buffers starting at d_src into `sl` and return: either one launch on a scan
// stream (scan, match and records in it, no event behind it: the host sees the summary land in mapped memory), or
// [reset ->] scan [-> carry update] there, match -> order -> records on the tail stream (or the scan stream) and, for a
// dense stream, score / emit on the score stream, `done` behind the last.  All results are written straight into the
// slot's mapped host memory: there is no copy back.
int enqueue_pass(adsb_ctx *c, Slot &sl, const void *d_src, SrcFormat fmt, uint64_t n_samples, uint32_t n_chunks,
                 const PassOptions &opt)
{
    PassPlan pl;
    if (int rc = plan_pass(c, sl, fmt, n_chunks, opt, pl)) return rc;
    ScanParams p{};
    fill_pass(c, sl, p, d_src, fmt, n_samples, n_chunks, opt, pl);
    if (int rc = order_behind_input(c, opt.input_done, pl.si, pl.ss)) return rc;   // edge in
    if (int rc = edges_before_scan(c, sl, p, pl)) return rc;             // edges 0, 1'', one launch: 1, 2, 3'
    if (int rc = enqueue_signal_stats(c, sl, p, fmt, opt, pl)) return rc;  // (no edge: stream order on the scan stream)
    // receiver seams (adsb_set_receiver_carry), only when the mode is on: the seam step in front of the scan launch, on its
    // stream and behind the same edges as the signal statistics (no edge of its own: every pass of the mode runs on the
    // first scan stream), and k_seam_match behind the pass's last kernel on the stream that one ran on
    if (int rc = seam_front(c, sl, p, fmt, pl.fast, opt.redo, pl.ss)) return rc;
    if (int rc = launch_scan_step(c, sl, p, fmt, opt, pl)) return rc;    // (row 6)
    if (pl.fused) {   // everything is out; what the next pass has to know about this one
        sl.tail_q = c->prev_scan_stream = pl.ss;
        c->prev_scanned = nullptr;
        c->prev_inline = c->prev_fused = true;
        return seam_tail(c, sl, pl.ss);
    }
    if (int rc = enqueue_tail(c, sl, p, fmt, pl)) return rc;             // edges 1, 2, 2', 3
    if (int rc = seam_tail(c, sl, sl.tail_q)) return rc;                 // (before `done`: edge 5 covers it)
    return enqueue_score(c, sl, p, pl);                                  // edges 4, 5
}

std::vector<uint32_t> filter_addresses(const adsb_ctx *c)
{
    std::vector<uint32_t> addrs;
    for (uint32_t a : c->filter.table())
        if (a != 0 && a <= 0xFFFFFFu) addrs.push_back(a);  // DF18 entries (addr | 1 << 25) match no 24-bit residual
    if (c->n_receivers > 1) {
        // the superset every receiver's buffers are matched against: the union of all their filters
        for (const IcaoFilter &f : c->rx_filters)
            for (uint32_t a : f.table())
                if (a != 0 && a <= 0xFFFFFFu) addrs.push_back(a);
        std::sort(addrs.begin(), addrs.end());
        addrs.erase(std::unique(addrs.begin(), addrs.end()), addrs.end());
    }
    return addrs;
}

// The exact bitmap rebuilt from the host's filter table (only while nothing is in flight).
int resync_exact(adsb_ctx *c)
{
    const std::vector<uint32_t> addrs = filter_addresses(c);
    hipStream_t ts = c->score_stream;
    for (uint32_t *bm : c->exact_bm) HIP_TRY(c, hipMemsetAsync(bm, 0, kBitmapAllocWords * sizeof(uint32_t), ts));
    if (!addrs.empty()) {
        if (int rc = ensure_addrs(c, addrs.size(), IcaoFilter::kSize)) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_addrs, addrs.data(), addrs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ts));
        if (int e = launch_set_addresses(c->d_addrs, (uint32_t)addrs.size(), c->exact_bm[c->cur_exact], kFullBitmapLg, ts))
            return fail(c, (hipError_t)e, "launch_set_addresses");
    }
    HIP_TRY(c, hipStreamSynchronize(ts));  // (rare: only after the host scored a pass itself)
    c->exact_valid = true;
    return ADSB_OK;
}

// The keyed set of a receivers context rebuilt from every receiver's host filter (only while nothing is in flight).  With
// an icao_flush pending the pass about to be planned starts from empty filters: both sets are emptied and none is filled.
// A rebuild that runs out of probes (more addresses than the capped set takes within its probe bound) leaves the set
// invalid and c->rx_set_full set: the host scores until the next icao_flush.
int rebuild_rx_set(adsb_ctx *c)
{
    hipStream_t ts = c->score_stream;
    c->rx_set_rebuilds++;
    c->rx_set_valid = false;
    for (auto *st : c->rx_set) HIP_TRY(c, hipMemsetAsync(st, 0xFF, sizeof(unsigned long long) << c->rx_set_alloc_lg, ts));
    std::vector<unsigned long long> keys;
    if (!c->flush_pending)
        for (uint32_t r = 0; r < c->n_receivers; r++)
            for (uint32_t a : c->rx_filter_of[r]->table())
                if (a != 0 && a <= 0xFFFFFFu) keys.push_back((unsigned long long)r << 24 | a);   // (DF18 entries match no 24-bit value)
    uint32_t failed = 0;
    if (!keys.empty()) {
        if (int rc = ensure_rx_keys(c, keys.size())) return rc;
        HIP_TRY(c, hipMemsetAsync(c->d_rx_failed, 0, sizeof(uint32_t), ts));
        HIP_TRY(c, hipMemcpyAsync(c->d_rx_keys, keys.data(), keys.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ts));
        if (int e = launch_rx_set_fill(c->d_rx_keys, (uint32_t)keys.size(), c->rx_set[c->cur_rx_set], c->rx_set_lg(), c->rx_probe_max(),
                                       c->d_rx_failed, ts))
            return fail(c, (hipError_t)e, "launch_rx_set_fill");
        HIP_TRY(c, hipMemcpyAsync(&failed, c->d_rx_failed, sizeof(uint32_t), hipMemcpyDeviceToHost, ts));
    }
    HIP_TRY(c, hipStreamSynchronize(ts));  // (rare: only after the host scored a pass itself, or a receiver flush)
    c->rx_set_full = failed != 0;
    c->rx_set_valid = failed == 0;
    return ADSB_OK;
}

// The overflow fallback re-runs a pass against the bitmap in use NOW.  Passes submitted after the
// overflowed one may have rotated the bitmaps (an icao_flush in between) and the retired one has been
// cleared, so the addresses the filter held before this pass would be missing from the superset:
// put them back.  At this point the host filter is exactly the state that preceded the pass (later
// passes have not been replayed yet), and extra bits only widen the superset for later passes.
int reseed_bitmap_from_filter(adsb_ctx *c)
{
    const std::vector<uint32_t> addrs = filter_addresses(c);
    if (addrs.empty()) return ADSB_OK;
    if (c->n_receivers) c->rx_reseeds++;
    // (one filter holds at most 4096 addresses; the union of many receivers' may hold more)
    if (int rc = ensure_addrs(c, addrs.size(), std::max<size_t>(IcaoFilter::kSize, addrs.size()))) return rc;
    HIP_TRY(c, hipMemcpy(c->d_addrs, addrs.data(), addrs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (int e = launch_set_addresses(c->d_addrs, (uint32_t)addrs.size(), c->d_bitmap[c->cur_bitmap], c->bitmap_lg, c->scan_stream[0]))
        return fail(c, (hipError_t)e, "launch_set_addresses");
    return ADSB_OK;
}

int submit(adsb_ctx *c, const void *d_src, SrcFormat fmt, uint64_t n_samples, bool inline_tail,
           hipEvent_t input_done)
{
    const uint64_t n_chunks = fmt == SrcFormat::kMag ? 1 : (n_samples + kChunkSamples - 1) / kChunkSamples;
    if (n_chunks == 0 || n_chunks > kMaxChunks || n_chunks > c->max_chunks) return ADSB_ERR_INVALID;
    Slot &sl = c->slot[c->submitted % (uint64_t)c->n_slots];
    if (sl.busy || sl.parked || c->shard_active) return ADSB_ERR_BUSY;
#ifdef ADSB_TUNING
    const auto te0 = std::chrono::steady_clock::now();
#endif
    PassOptions opt;
    opt.inline_tail = inline_tail;
    opt.input_done = input_done;
    if (c->n_receivers) {
        // whose buffers these are: the caller's map from this pass's first buffer on (a blocking call cut into passes
        // hands it on piece by piece), or receiver 0 throughout for a plain call (within the capacity reserved by
        // adsb_set_receivers: nothing is allocated).  In front of the enqueue: a pass scored on the device takes it along.
        if (c->rx_call_map) sl.rx_map.assign(c->rx_call_map, c->rx_call_map + n_chunks);
        else sl.rx_map.assign((size_t)n_chunks, 0u);
    }
    int rc = enqueue_pass(c, sl, d_src, fmt, n_samples, (uint32_t)n_chunks, opt);
#ifdef ADSB_TUNING
    c->t_enqueue += std::chrono::duration<double>(std::chrono::steady_clock::now() - te0).count();
#endif
    if (rc) return rc;
    if (c->n_receivers) {
        if (c->rx_call_map) c->rx_call_map += n_chunks;
        // ... and the receiver flushes asked for since the previous submission (a pass scored on the device that had to
        // rebuild its keyed set has applied them already: plan_pass)
        sl.rx_flush.clear();
        sl.rx_flush.swap(c->rx_flush_next);
    }
    sl.busy = true;
    c->submitted++;
    return ADSB_OK;
}

// synchronous pass: everything pending is finished first, in order
int run_sync(adsb_ctx *c, const void *d_src, SrcFormat fmt, uint64_t n_samples, std::vector<adsb_msg> &out,
             hipEvent_t input_done)
{
    if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
    int rc = submit(c, d_src, fmt, n_samples, true, input_done);
    if (rc) return rc;
    return collect_next(c, out);
}

// A long stream goes in pieces: the messages of the piece at sample `off` (chunk = buffer of the stream) and the
// stats its pass left in the context join the call's.
void append_piece(const adsb_ctx *c, std::vector<adsb_msg> &part, uint64_t off, std::vector<adsb_msg> &out, adsb_stats &total,
                         std::vector<adsb_signal_stats> &sig)
{
    for (auto &m : part) {
        m.chunk += off / kChunkSamples;
        out.push_back(m);
    }
    for (adsb_signal_stats r : c->sig_out) {   // (the piece's signal records, when the mode is on)
        r.chunk += off / kChunkSamples;
        sig.push_back(r);
    }
    const adsb_stats &st = c->stats;
    total.n_chunks += st.n_chunks, total.n_candidates += st.n_candidates, total.n_ap_entries += st.n_ap_entries;
    total.n_records += st.n_records, total.ms_scan += st.ms_scan, total.ms_scan_exclusive += st.ms_scan_exclusive;
    total.ms_match += st.ms_match, total.ms_records += st.ms_records, total.ms_total_device += st.ms_total_device;
    total.retries += st.retries;
}

// IQ stream of any length resident on the device.
int demod_device(adsb_ctx *c, const void *d_iq, uint64_t n_samples, std::vector<adsb_msg> &out, SrcFormat fmt)
{
    if (n_samples == 0) {
        c->stats = adsb_stats{};
        c->sig_out.clear();
        return ADSB_OK;
    }
    adsb_stats total{};
    std::vector<adsb_signal_stats> sig;
    // a device pass takes at most max_chunks buffers (what the context's lists were sized for;
    // never more than kMaxChunks: entry packing): longer streams go in pieces, which is what
    // consecutive calls would be -- buffers are independent but for the filter
    const uint64_t piece = std::min<uint64_t>(kMaxChunks, c->max_chunks) * (uint64_t)kChunkSamples;
    for (uint64_t off = 0; off < n_samples; off += piece) {
        const uint64_t n = std::min<uint64_t>(piece, n_samples - off);
        std::vector<adsb_msg> part;
        int rc = run_sync(c, (const char *)d_iq + off * src_bytes_per_sample(fmt), fmt, n, part);
        if (rc) return rc;
        append_piece(c, part, off, out, total, sig);
    }
    total.n_samples = n_samples;
    c->stats = total;
    c->sig_out.swap(sig);
    return ADSB_OK;
}

void soapy_u8_table(int16_t *out256)
{
    // float32 at every step and a truncating conversion, as SoapyRTLSDR builds its lookup table
    for (int x = 0; x < 256; x++) {
        volatile float v = (float)x - 127.4f;   // (volatile: one rounding per operation, never contracted)
        v = v * (1.0f / 128.0f);
        v = v * 32767.0f;
        out256[x] = (int16_t)v;
    }
}

namespace {
int to_mag_host(adsb_ctx *c, const void *iq, size_t n, uint16_t *data_out, size_t *length_out, SrcFormat fmt)
{
    if (!c || (!iq && n) || !data_out) return ADSB_ERR_INVALID;
    if (n > kChunkSamples) return ADSB_ERR_TOO_LONG;  // reference: index panic, lib.rs:48
    ADSB_ON_DEVICE(c);
    // Through pinned, mapped memory both ways: one host copy in, the kernel reads the samples and writes
    // the 131398 magnitudes in place over the link, one host copy out -- instead of two copy commands
    // from / to pageable memory with their staging inside the runtime (62 -> ~36 us for the reference's
    // own buffer size).
    const size_t in_bytes = (size_t)kChunkSamples * 4, out_bytes = (size_t)kMagDataLen * sizeof(uint16_t);
    const size_t out_off = (in_bytes + 255) & ~(size_t)255;
    if (int rc = ensure_host_stage(c, out_off + out_bytes)) return rc;
    if (n) std::memcpy(c->h_stage, iq, n * src_bytes_per_sample(fmt));
    uint16_t *h_mag = reinterpret_cast<uint16_t *>((char *)c->h_stage + out_off);
    uint16_t *h_mag_dev = reinterpret_cast<uint16_t *>((char *)c->h_stage_dev + out_off);
    if (int e = launch_to_mag(c->h_stage_dev, (uint32_t)n, h_mag_dev, c->stream,
                                fmt == SrcFormat::kCu8 ? c->d_u8_table : nullptr))
        return fail(c, (hipError_t)e, "launch_to_mag");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::memcpy(data_out, h_mag, out_bytes);
    if (length_out) *length_out = n;
    return ADSB_OK;
}

int demod_device_entry(adsb_ctx *c, const void *d_iq, size_t n_samples, adsb_msg *out, size_t cap, size_t *n_out, SrcFormat fmt)
{
    if (!c || (!d_iq && n_samples) || (!out && cap)) return ADSB_ERR_INVALID;
    if (((uintptr_t)d_iq & 15u) != 0) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(c);
    std::vector<adsb_msg> msgs;
    int rc = demod_device(c, d_iq, n_samples, msgs, fmt);
    if (rc) return rc;
    return deliver(c, msgs, out, cap, n_out);
}

int submit_device_entry(adsb_ctx *c, const void *d_iq, size_t n_samples, SrcFormat fmt)
{
    if (!c || !d_iq || n_samples == 0) return ADSB_ERR_INVALID;
    if (((uintptr_t)d_iq & 15u) != 0) return ADSB_ERR_INVALID;
    if ((n_samples + kChunkSamples - 1) / kChunkSamples > std::min<uint64_t>(kMaxChunks, c->max_chunks))
        return ADSB_ERR_INVALID;  // more buffers than the context was created for
    ADSB_ON_DEVICE(c);
    return submit(c, d_iq, fmt, n_samples);
}

// adsb_demod_iq / adsb_demod_iq_u8: a host IQ stream of either format (bps bytes per sample)
int demod_host(adsb_ctx *c, const void *iq, size_t n_samples, adsb_msg *out, size_t cap, size_t *n_out, SrcFormat fmt)
{
    if (!c || (!iq && n_samples) || (!out && cap)) return ADSB_ERR_INVALID;
    const size_t bps = src_bytes_per_sample(fmt);
    const char *iqb = static_cast<const char *>(iq);
    ADSB_ON_DEVICE(c);
    // stage through the device in pieces of at most max_chunks chunks
    std::vector<adsb_msg> msgs;
    adsb_stats total{};
    std::vector<adsb_signal_stats> sig;
    if (c->submitted == c->delivered) c->sig_out.clear();   // (a call of no samples runs no pass: no records)
    const size_t piece = c->max_chunks * (size_t)kChunkSamples;
    // A call of a few buffers (the reference's own call shape, benches/demod_benchmark.rs:10-11: one
    // 131072-sample buffer) is one launch that reads the samples in place from pinned host memory: one
    // host copy into it instead of a copy command, its staging inside the runtime and an event.
    // Samples inside a buffer the caller registered (adsb_host_register) are pinned and mapped already: one launch
    // that reads them where they are, no host copy at all.
    if (n_samples && n_samples <= std::min<size_t>(piece, (size_t)kInlineTailChunks * kChunkSamples) && !ordered_passes(c) &&
        ((uintptr_t)iq & 15u) == 0) {
        const char *b = iqb;
        for (const auto &r : c->host_ranges)
            if (b >= r.base && b + n_samples * bps <= r.base + r.bytes) {
                if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
                int rc = run_sync(c, r.dev + (b - r.base), fmt, n_samples, msgs, input_ready_now());
                if (rc) return rc;
                c->stats.n_samples = n_samples;
                return deliver(c, msgs, out, cap, n_out);
            }
    }
    const bool in_place = n_samples <= (size_t)kInlineTailChunks * kChunkSamples && !ordered_passes(c);
    int rc = in_place ? ensure_host_stage(c, std::max<size_t>(n_samples, 1) * bps + 512)   // (+ the progress word)
                      : ensure_stage(c, std::min(piece, std::max<size_t>(n_samples, 1)) * bps);
    if (rc) return rc;
    // (not with signal statistics on: k_signal_stats goes out in front of the scan and waits for no progress word)
    if (in_place && n_samples && n_samples <= piece && !c->signal_stats &&
        one_launch_pass(c, (uint32_t)((n_samples + kChunkSamples - 1) / kChunkSamples))) {
        // One pass of one launch: launch it FIRST and copy the samples into the pinned buffer while the launch is on its way
        // (dispatch latency ~5 us, the copy ~10): each workgroup waits for the host's progress word to pass the
        // end of its tile (ScanParams::src_ready), so the copy and the first tiles overlap instead of adding up.
        const size_t ready_off = (n_samples * bps + 255) & ~(size_t)255;
        if (int rc2 = ensure_host_stage(c, ready_off + 64)) return rc2;
        unsigned long long *ready = reinterpret_cast<unsigned long long *>((char *)c->h_stage + ready_off);
        __atomic_store_n(ready, 0ull, __ATOMIC_RELEASE);
        if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
        c->next_src_ready = reinterpret_cast<const unsigned long long *>((char *)c->h_stage_dev + ready_off);
        rc = submit(c, c->h_stage_dev, fmt, n_samples, true, input_ready_now());
        c->next_src_ready = nullptr;
        // (whatever submit said, the copy is finished before anything else: a pass that was launched reads it)
        constexpr size_t kStep = 16384;   // samples per progress update: two tiles
        for (size_t done = 0; done < n_samples;) {
            const size_t k = std::min(kStep, n_samples - done);
            std::memcpy((char *)c->h_stage + done * bps, iqb + done * bps, k * bps);
            done += k;
            __atomic_store_n(ready, (unsigned long long)done, __ATOMIC_RELEASE);
        }
        if (rc) return rc;
        rc = collect_next(c, msgs);
        if (rc) return rc;
        c->stats.n_samples = n_samples;
        return deliver(c, msgs, out, cap, n_out);
    }
    if (in_place && n_samples) {
        std::memcpy(c->h_stage, iqb, n_samples * bps);
        for (size_t off = 0; off < n_samples; off += piece) {
            const size_t n = std::min(piece, n_samples - off);
            std::vector<adsb_msg> part;
            rc = run_sync(c, (const char *)c->h_stage_dev + off * bps, fmt, n, part, input_ready_now());
            if (rc) return rc;
            append_piece(c, part, off, msgs, total, sig);
        }
        total.n_samples = n_samples;
        c->stats = total;
        c->sig_out.swap(sig);
        return deliver(c, msgs, out, cap, n_out);
    }
    for (size_t off = 0; off < n_samples; off += piece) {
        const size_t n = std::min(piece, n_samples - off);
        HIP_TRY(c, hipMemcpyAsync(c->d_stage, iqb + off * bps, n * bps, hipMemcpyHostToDevice, c->stream));
        c->own_stream_dirty = true;
        std::vector<adsb_msg> part;
        rc = demod_device(c, c->d_stage, n, part, fmt);
        if (rc) return rc;
        append_piece(c, part, off, msgs, total, sig);
    }
    total.n_samples = n_samples;
    c->stats = total;
    c->sig_out.swap(sig);
    return deliver(c, msgs, out, cap, n_out);
}
}  // namespace

}  // namespace host
}  // namespace adsb

extern "C" {

int adsb_to_mag(adsb_ctx *c, const int16_t *iq, size_t n, uint16_t *data_out, size_t *length_out)
try {
    return to_mag_host(c, iq, n, data_out, length_out, SrcFormat::kCs16);
} ADSB_ABI_CATCH

int adsb_to_mag_u8(adsb_ctx *c, const uint8_t *iq, size_t n, uint16_t *data_out, size_t *length_out)
try {
    return to_mag_host(c, iq, n, data_out, length_out, SrcFormat::kCu8);
} ADSB_ABI_CATCH

int adsb_demodulate2400(adsb_ctx *c, const uint16_t *data, size_t length, adsb_msg *out, size_t cap,
                        size_t *n_out)
try {
    if (!c || !data || (!out && cap)) return ADSB_ERR_INVALID;
    if (length > kChunkSamples) return ADSB_ERR_TOO_LONG;
    ADSB_ON_DEVICE(c);
    if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
    c->stats = adsb_stats{};
    c->stats.n_samples = length;
    c->stats.n_chunks = 1;
    c->sig_out.clear();   // (the caller's magnitudes: no signal records)
    std::vector<adsb_msg> msgs;
    if (length) {
        // the caller's MagnitudeBuffer into pinned memory; the pass (one launch) reads it in place
        const size_t bytes = (size_t)kMagDataLen * sizeof(uint16_t);
        if (int rc = ensure_host_stage(c, bytes)) return rc;
        std::memcpy(c->h_stage, data, bytes);
        int rc = run_sync(c, c->h_stage_dev, SrcFormat::kMag, length, msgs, input_ready_now());
        if (rc) return rc;
    }
    return deliver(c, msgs, out, cap, n_out);
} ADSB_ABI_CATCH

int adsb_demod_iq_device(adsb_ctx *c, const void *d_iq, size_t n_samples, adsb_msg *out, size_t cap,
                         size_t *n_out)
try {
    return demod_device_entry(c, d_iq, n_samples, out, cap, n_out, SrcFormat::kCs16);
} ADSB_ABI_CATCH

int adsb_demod_iq_device_u8(adsb_ctx *c, const void *d_iq, size_t n_samples, adsb_msg *out, size_t cap, size_t *n_out)
try {
    return demod_device_entry(c, d_iq, n_samples, out, cap, n_out, SrcFormat::kCu8);
} ADSB_ABI_CATCH

int adsb_submit_iq_device(adsb_ctx *c, const void *d_iq, size_t n_samples)
try {
    return submit_device_entry(c, d_iq, n_samples, SrcFormat::kCs16);
} ADSB_ABI_CATCH

int adsb_submit_iq_device_u8(adsb_ctx *c, const void *d_iq, size_t n_samples)
try {
    return submit_device_entry(c, d_iq, n_samples, SrcFormat::kCu8);
} ADSB_ABI_CATCH

// ---- many receivers, one pass: the calls above with the receiver of every buffer (rx_check: the mode is on and the
// whole map is valid, before anything is enqueued or any filter touched; RxCall: the passes of this call take it) ----
int adsb_demod_iq_rx(adsb_ctx *c, const int16_t *iq, size_t n_samples, const uint32_t *receiver_of_buffer, adsb_msg *out,
                     size_t cap, size_t *n_out)
try {
    if (int rc = rx_check(c, n_samples, receiver_of_buffer)) return rc;
    RxCall call(c, receiver_of_buffer);
    return demod_host(c, iq, n_samples, out, cap, n_out, SrcFormat::kCs16);
} ADSB_ABI_CATCH

int adsb_demod_iq_rx_u8(adsb_ctx *c, const uint8_t *iq, size_t n_samples, const uint32_t *receiver_of_buffer, adsb_msg *out,
                        size_t cap, size_t *n_out)
try {
    if (int rc = rx_check(c, n_samples, receiver_of_buffer)) return rc;
    RxCall call(c, receiver_of_buffer);
    return demod_host(c, iq, n_samples, out, cap, n_out, SrcFormat::kCu8);
} ADSB_ABI_CATCH

int adsb_demod_iq_device_rx(adsb_ctx *c, const void *d_iq, size_t n_samples, const uint32_t *receiver_of_buffer, adsb_msg *out,
                            size_t cap, size_t *n_out)
try {
    if (int rc = rx_check(c, n_samples, receiver_of_buffer)) return rc;
    RxCall call(c, receiver_of_buffer);
    return demod_device_entry(c, d_iq, n_samples, out, cap, n_out, SrcFormat::kCs16);
} ADSB_ABI_CATCH

int adsb_demod_iq_device_rx_u8(adsb_ctx *c, const void *d_iq, size_t n_samples, const uint32_t *receiver_of_buffer,
                               adsb_msg *out, size_t cap, size_t *n_out)
try {
    if (int rc = rx_check(c, n_samples, receiver_of_buffer)) return rc;
    RxCall call(c, receiver_of_buffer);
    return demod_device_entry(c, d_iq, n_samples, out, cap, n_out, SrcFormat::kCu8);
} ADSB_ABI_CATCH

int adsb_submit_iq_device_rx(adsb_ctx *c, const void *d_iq, size_t n_samples, const uint32_t *receiver_of_buffer)
try {
    if (int rc = rx_check(c, n_samples, receiver_of_buffer)) return rc;
    RxCall call(c, receiver_of_buffer);
    return submit_device_entry(c, d_iq, n_samples, SrcFormat::kCs16);
} ADSB_ABI_CATCH

int adsb_submit_iq_device_rx_u8(adsb_ctx *c, const void *d_iq, size_t n_samples, const uint32_t *receiver_of_buffer)
try {
    if (int rc = rx_check(c, n_samples, receiver_of_buffer)) return rc;
    RxCall call(c, receiver_of_buffer);
    return submit_device_entry(c, d_iq, n_samples, SrcFormat::kCu8);
} ADSB_ABI_CATCH

int adsb_demod_iq(adsb_ctx *c, const int16_t *iq, size_t n_samples, adsb_msg *out, size_t cap,
                  size_t *n_out)
try {
    return demod_host(c, iq, n_samples, out, cap, n_out, SrcFormat::kCs16);
} ADSB_ABI_CATCH

int adsb_demod_iq_u8(adsb_ctx *c, const uint8_t *iq, size_t n_samples, adsb_msg *out, size_t cap, size_t *n_out)
try {
    return demod_host(c, iq, n_samples, out, cap, n_out, SrcFormat::kCu8);
} ADSB_ABI_CATCH

}  // extern "C"
