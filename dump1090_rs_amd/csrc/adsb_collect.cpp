// adsb_collect.cpp -- waiting for a pass, its checksums, the ordered host replay (src/demod_2400.rs:149-207 with
// src/mode_s/mod.rs:34-139 scoring against src/icao_filter.rs), and the overflow fallback.
#include "adsb_ctx.h"

using namespace adsb::host;

namespace {

// the 64-bit sum of n 8-byte words of mapped host memory that the device may still be writing: the checksum the
// kernels keep of their records and of their messages
uint64_t word_sum(const void *p, size_t n)
{
    const uint64_t *w = static_cast<const uint64_t *>(p);
    uint64_t got = 0;
    for (size_t i = 0; i < n; i++) got += __atomic_load_n(&w[i], __ATOMIC_RELAXED);
    return got;
}

// ---- the two things a plain pass and a receivers pass do differently with a device result: the room test, and where
// the additions go.  A filter that is nearly full is the one situation whose reference behaviour (icao_filter_add gives
// up on a full table, src/icao_filter.rs:46-62) the parallel formulation does not reproduce. ----
bool adds_have_room(adsb_ctx *c, size_t na)
{
    size_t held = 0;
    for (uint32_t a : c->filter.table()) held += a != 0;
    return held + na + 64 < IcaoFilter::kSize;
}

// the distinct values among receiver r's additions of the pass
size_t distinct_adds_rx(adsb_ctx *c, const Slot &sl, size_t na, uint32_t r)
{
    std::vector<uint32_t> &v = c->rx_add_values;
    v.clear();
    for (size_t i = 0; i < na; i++)
        if (sl.h_add_rx[i] == r) v.push_back(sl.h_adds[i]);
    std::sort(v.begin(), v.end());
    return (size_t)(std::unique(v.begin(), v.end()) - v.begin());
}

// ... for EVERY receiver that has an addition in the pass (sl.h_add_rx: the receiver of each) -- held[r] + adds[r] + 64
// < 4096, with held[r] kept from pass to pass and counted afresh whenever the host has touched the filters itself.  The
// list has one entry per add() CALL (a DF18 whose plain address is unknown re-adds address | NT on every frame and
// phase), the table one per distinct value: a receiver whose calls alone would not fit has its distinct values counted
// (as adsb_multi.cpp's fits() does), so that a long pass of few receivers is not refused for its repetitions.
bool adds_have_room_rx(adsb_ctx *c, const Slot &sl, size_t na)
{
    if (!c->rx_held_valid) {
        c->rx_held.assign(c->n_receivers, 0u);
        c->rx_pass_adds.assign(c->n_receivers, 0u);
        for (uint32_t r = 0; r < c->n_receivers; r++)
            for (uint32_t a : c->rx_filter_of[r]->table()) c->rx_held[r] += a != 0;
        c->rx_held_valid = true;
    }
    bool room = true;
    c->rx_touched.clear();
    for (size_t i = 0; i < na && room; i++) {
        const uint32_t r = sl.h_add_rx[i];
        if (r >= c->n_receivers) room = false;   // (not a receiver: not this pass's whole result)
        else if (c->rx_pass_adds[r]++ == 0) c->rx_touched.push_back(r);
    }
    for (uint32_t r : c->rx_touched) {
        if (room && (size_t)c->rx_held[r] + c->rx_pass_adds[r] + 64 >= IcaoFilter::kSize)
            room = (size_t)c->rx_held[r] + distinct_adds_rx(c, sl, na, r) + 64 < IcaoFilter::kSize;
        c->rx_pass_adds[r] = 0;
    }
    return room;
}

// the pass's additions into the host's filter, in order; true: it took a new address
bool apply_adds(adsb_ctx *c, const Slot &sl, size_t na)
{
    const uint64_t before = c->filter.inserts();
    for (size_t i = 0; i < na; i++) c->filter.add(sl.h_adds[i]);
    return c->filter.inserts() != before;
}

bool apply_adds_rx(adsb_ctx *c, const Slot &sl, size_t na)
{
    bool gained = false;
    for (size_t i = 0; i < na; i++) {
        const uint32_t r = sl.h_add_rx[i];
        IcaoFilter &f = *c->rx_filter_of[r];
        const uint64_t before = f.inserts();
        f.add(sl.h_adds[i]);
        if (f.inserts() != before) {
            c->rx_held[r]++;
            gained = true;
        }
    }
    return gained;
}

// The pass's messages as the device scored them, when they can be taken as they are: scored in the current epoch, with
// room in the filter (one, or one per receiver: sl.rx_scored, a pass of the keyed kernels of adsb_score_rx.hip, whose
// additions come as (value, receiver) pairs), and whole (checksum).  Applies the pass's additions to the host's filters.
bool take_device_result(adsb_ctx *c, Slot &sl, uint64_t chunk_offset, std::vector<adsb_msg> &out)
{
    const bool rx = sl.rx_scored;   // (implies device_scored: fill_pass)
    if (!sl.device_scored) return false;
    // (receiver seams scored on the device: the merge ran, whatever becomes of its result -- counted from its own summary,
    // behind the pass's `done`, also for a pass that is disowned below)
    count_seam_merge(c, sl);
    if (sl.score_epoch != c->score_epoch) return false;
    const ScoreSummary *ss = sl.h_ssum;
    if (__atomic_load_n(&ss->seq, __ATOMIC_ACQUIRE) != sl.seq) return false;
    if (rx && ss->no_room) c->rx_no_room++;   // (counted whether or not the pass says it was scored: it never does then)
    if (!ss->scored) return false;
    const size_t nm = ss->n_msgs, na = ss->n_adds;
    if (nm > c->score.cap || na > c->score.cap) return false;
    if (!(rx ? adds_have_room_rx(c, sl, na) : adds_have_room(c, na))) return false;
    const uint64_t want = (uint64_t)ss->msg_sum_hi << 32 | ss->msg_sum_lo;
    bool whole = false;
    for (int attempt = 0; attempt < 200 && !whole; attempt++) whole = word_sum(sl.h_msgs, 5 * nm) == want;
    if (!whole) return false;
    const size_t at = out.size();
    out.insert(out.end(), sl.h_msgs, sl.h_msgs + nm);
    if (chunk_offset)
        for (size_t i = at; i < out.size(); i++) out[i].chunk += chunk_offset;
    if (rx ? apply_adds_rx(c, sl, na) : apply_adds(c, sl, na)) c->last_new_insert_seq = sl.scan_seq;
    c->rx_scored_taken += rx;
    return true;
}

// The ordered replay of a pass whose buffers belong to several receivers (adsb_set_receivers): every record against the
// filter of the receiver of its buffer, sl.rx_map[chunk_offset + chunk] (chunk_offset: the buffer the overflow fallback
// is at).  A pass of at least rx_parallel_min records with more than one receiver in it is dealt, receiver by receiver,
// to the threads of a pool made when the first such pass comes along (adsb_replay_host.h: ReceiverReplay).
// *gained: some receiver's filter took a new address.
int replay_receivers(adsb_ctx *c, const Slot &sl, const TrialRecord *rec, size_t n, uint64_t chunk_offset, std::vector<adsb_msg> &out,
                     bool *gained)
{
    const size_t first = (size_t)chunk_offset, last = std::min(sl.rx_map.size(), first + sl.n_chunks);
    bool several = false;
    for (size_t b = first + 1; b < last && !several; b++) several = sl.rx_map[b] != sl.rx_map[first];
    ReplayPool *pool = nullptr;
    if (several && n >= c->rx_parallel_min) {
        if (!c->rx_pool) {
            // up to six threads beside the caller, never more than a quarter of the cores; they sleep between passes
            const unsigned hw = std::thread::hardware_concurrency();
            c->rx_pool.reset(new ReplayPool((int)std::min(6u, std::max(1u, hw / 4)), {}, 0));
        }
        pool = c->rx_pool.get();
    }
    bool pooled = false;
    if (!c->rx_replay.run(c->rx_filter_of.data(), sl.rx_map.data(), sl.rx_map.size(), c->crc, rec, n, chunk_offset, out, pool,
                          &c->host_sorts, gained, &pooled)) {
        c->last_error = "a trial record names a buffer outside the pass that wrote it";
        return ADSB_ERR_HIP;
    }
    c->rx_passes++;
    c->rx_pooled += pooled;
    return ADSB_OK;
}

}  // namespace

namespace adsb {
namespace host {

void flush_host_filters(adsb_ctx *c)
{
    c->filter.flush();
    for (IcaoFilter &f : c->rx_filters) f.flush();
    std::fill(c->rx_held.begin(), c->rx_held.end(), 0u);   // (adds_have_room_rx's counts, while they are valid: all empty)
}

// adsb_icao_flush_receiver calls that waited for their pass: the host's filters and the counts of what they hold (host
// only: the device's superset stays one)
void flush_receivers(adsb_ctx *c, std::vector<uint32_t> &receivers)
{
    for (uint32_t r : receivers)
        if (r < c->rx_filter_of.size()) {
            c->rx_filter_of[r]->flush();
            if (r < c->rx_held.size()) c->rx_held[r] = 0;
        }
    receivers.clear();
}

// The records and the summary travel to host memory as separate posted writes; the summary's
// sequence word says the pass is done, this says every one of its records has landed whole: the
// 64-bit sum of all their u64 words, as the records kernel added them up.  (Records that are still
// in flight when the completion event has fired would be a platform fault: give them a moment,
// then fail loudly rather than replay something torn.)
int verify_records(adsb_ctx *c, const Summary *sum, const TrialRecord *rec, size_t n)
{
    const uint64_t want = (uint64_t)sum->rec_sum_hi << 32 | sum->rec_sum_lo;
    for (int attempt = 0; attempt < 200; attempt++) {
        if (word_sum(rec, 4 * n) == want) return ADSB_OK;
        for (volatile int spin = 0; spin < 2000; spin++) {}
    }
    if (c) c->last_error = "trial records in host memory do not add up to the checksum of the pass that wrote them";
    return ADSB_ERR_HIP;
}

// The summary is ten separate posted writes with the sequence word issued last; a host that polls for it
// takes the summary only when its own checksum covers what it reads (a word that overtook its neighbours
// on the way would otherwise pair this pass's sequence number with the previous pass's counts).
bool summary_landed(const Summary *s, uint32_t seq)
{
    if (__atomic_load_n(&s->seq, __ATOMIC_ACQUIRE) != seq) return false;
    uint32_t w[10];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(s);
    for (int k = 0; k < 10; k++) w[k] = __atomic_load_n(&src[k], __ATOMIC_RELAXED);
    return w[7] == seq && summary_check(w) == w[9];
}

// The signal records of the pass in `sl` (adsb_set_signal_stats) out of the slot's mapped memory into c->sig_out.  They
// were written by a kernel in front of the pass's scan on the scan's own stream, so they are there when the pass's summary
// is: one look, no waiting.  That look is a real check all the same: the records were overwritten with ones when the pass
// was enqueued, and no 8-byte word of a record can be all ones (a buffer index below 2^19, a sum below 2^49, counts of at
// most 131072) -- so a record with such a word, with another buffer's index or sample count, or whose histogram does not
// add up to its samples is not this pass's whole record, and the pass fails loudly instead of reporting it.
int take_signal_records(adsb_ctx *c, const Slot &sl)
{
    c->sig_out.resize(sl.n_chunks);
    for (uint32_t i = 0; i < sl.n_chunks; i++) {
        const uint64_t left = sl.n_samples - (uint64_t)i * kChunkSamples;
        const uint32_t want_n = (uint32_t)std::min<uint64_t>(left, kChunkSamples);
        adsb_signal_stats r;
        const uint64_t *w = reinterpret_cast<const uint64_t *>(&sl.h_sig[i]);
        uint64_t *d = reinterpret_cast<uint64_t *>(&r);
        bool whole = true;
        for (size_t k = 0; k < sizeof(r) / 8; k++) {
            d[k] = __atomic_load_n(&w[k], __ATOMIC_RELAXED);
            whole = whole && d[k] != ~0ull;
        }
        uint64_t in_bins = 0;
        for (uint32_t h : r.hist) in_bins += h;
        if (!whole || r.chunk != i || r.n_samples != want_n || in_bins != want_n) {
            c->sig_out.clear();
            c->last_error = "signal records in host memory are not the whole records of the pass that wrote them";
            return ADSB_ERR_HIP;
        }
        c->sig_out[i] = r;
    }
    return ADSB_OK;
}

// Wait for the pass in `sl` and replay it.  Returns 1 when a device list overflowed
// (caller re-runs in smaller pieces), 0 on success, < 0 on error.
int finish_pass(adsb_ctx *c, Slot &sl, uint64_t chunk_offset, adsb_stats &st, std::vector<adsb_msg> &out)
{
#ifdef ADSB_TUNING
    const auto tw0 = std::chrono::steady_clock::now();
#endif
    {
        HT(c, HT_SYNC);
        if (sl.fused) {
            // A one-launch pass has no event behind it: its last workgroup writes the summary into mapped
            // host memory (after the records, with their checksum), and that is what the host watches for.
            // Give up spinning after a while (a pass queued behind long ones) and block on its stream.
            const auto t0 = std::chrono::steady_clock::now();
            bool seen = false;
            for (uint32_t spin = 0; !seen; spin++) {
                seen = summary_landed(sl.h_sum, sl.seq);
                if (seen) break;
                __builtin_ia32_pause();
                if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
            }
            if (!seen) HIP_TRY(c, hipStreamSynchronize(sl.tail_q));
        } else {
            HIP_TRY(c, hipEventSynchronize(sl.done));
        }
    }
#ifdef ADSB_TUNING
    c->t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw0).count();
#endif
    {
        // (behind an event or a stream synchronisation every word has landed; the retries are for the
        // polled case that fell through to the stream wait with the last words still on their way)
        bool whole = false;
        for (int attempt = 0; attempt < 200 && !whole; attempt++) {
            whole = summary_landed(sl.h_sum, sl.seq);
            if (!whole) for (volatile int spin = 0; spin < 2000; spin++) {}
        }
        if (!whole) {
            c->last_error = "pass completed without publishing a whole summary";
            return ADSB_ERR_HIP;
        }
    }
    if (sl.h_sum->overflow) return 1;
    // A one-launch pass did not wait for the passes that were in flight on the other scan stream.  If one
    // of those (all replayed by now: passes are collected in order) taught the filter a NEW address, this
    // pass's address/parity trials may have been matched before its bit was set: again, through the three
    // launches (every earlier pass is complete now, so nothing can be missed a second time).
    if (sl.fused && sl.unsynced_from && c->last_new_insert_seq >= sl.unsynced_from) return 2;
    // Receiver seams: the seam step's records, once per pass (the overflow fallback's one-buffer passes find them taken;
    // so does a pass whose seam collect_oldest redid).  Its k_seam_match ran behind the pass's last kernel.
    // (A pass whose seam records were merged on the device, sl.seam_scored, needs them on the host only when its device
    // result is refused: below, then.)
    if (sl.seam_on && !c->seam_taken && !sl.seam_scored)
        if (int rc = take_seam(c, sl)) return rc;
    const size_t n = sl.h_sum->n_hits;
    // (k_records' own test: a pass that k_score took over has left its records in device memory)
    const bool rec_on_device = sl.device_scored && n <= c->score.cap;
    if (!rec_on_device) {
        HT(c, HT_VERIFY);
        if (int rc = verify_records(c, sl.h_sum, sl.h_rec, n)) return rc;
    }
    if (sl.profiled && sl.fused) {
        // a one-launch pass timed itself (device wall clock, 100 MHz): no events, nothing to wait for
        const float ms = (float)sl.h_sum->ticks * 1e-5f;
        st.ms_scan += ms;
        st.ms_scan_exclusive += ms;
    } else if (sl.profiled) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, sl.ev[0], sl.ev[1]));
        st.ms_scan += ms;
        // The device time this launch adds: the part of it after the latest scan end seen so far (the
        // "frontier": normally the previous pass's; scans on the two scan streams can also finish out of
        // order, and one that ended before the frontier adds nothing -- the union of the launches'
        // intervals is what is being summed).  The frontier's events are intact for kScanEvRing - n_slots
        // passes back: the ring is that much longer than what can be in flight.
        float excl = ms;
        bool advance = !sl.redo;   // (a pass run again is blocking and on events of its own: no part of the frontier)
        if (!sl.redo && c->last_stop && sl.scan_seq - c->last_scan_seq <= (uint64_t)(kScanEvRing - c->n_slots)) {
            float since = 0;
            if (hipEventElapsedTime(&since, c->last_stop, sl.ev[1]) == hipSuccess) {
                if (since <= 0) {
                    excl = 0;
                    advance = false;
                } else if (since < excl) {
                    excl = since;
                }
            }
        }
        st.ms_scan_exclusive += excl;
        if (advance) {
            c->last_stop = sl.ev[1];
            c->last_scan_seq = sl.scan_seq;
        }
        if (sl.profiled > 1) {  // per-kernel split of the tail (events cost a few us each)
            HIP_TRY(c, hipEventElapsedTime(&ms, sl.ev[2], sl.ev[3]));
            st.ms_match += ms;
            HIP_TRY(c, hipEventElapsedTime(&ms, sl.ev[3], sl.ev[4]));
            st.ms_records += ms;
            HIP_TRY(c, hipEventElapsedTime(&ms, sl.ev[0], sl.ev[4]));
            st.ms_total_device += ms;
        }
    }
    st.n_candidates += sl.h_sum->n_cand_total;
    st.n_ap_entries += sl.h_sum->n_ap_total;
    st.n_records += n;
    // Density is records per buffer (8 and more: device-side order + score; under 2: the host does
    // it), so that a context of 64 buffers decides like one of 512.  Passes too small to be ordered on
    // the device anyway (and the fallback's one-buffer passes) say nothing about the stream: a small
    // pass between large dense ones must not flip the mode, each flip drains the pipeline.
    if (sl.hits_cap == c->hits_cap && sl.n_chunks > kInlineTailChunks) {
        if (n >= 8u * (size_t)sl.n_chunks) c->dense_mode = true;
        else if (n < 2u * (size_t)sl.n_chunks) c->dense_mode = false;
    }
    // (a merged pass taken from the device: the host neither merges nor replays its seam records)
    if (take_device_result(c, sl, chunk_offset, out)) return 0;
    if (sl.rx_scored) c->rx_scored_refused++;
    if (sl.seam_on && !c->seam_taken)   // (sl.seam_scored and refused: the seam records after all, redone where they overflowed)
        if (int rc = take_seam(c, sl)) return rc;
    if (rec_on_device && n) {
        HIP_TRY(c, hipMemcpy(sl.h_rec, sl.score.rec, n * sizeof(TrialRecord), hipMemcpyDeviceToHost));
        if (int rc = verify_records(c, sl.h_sum, sl.h_rec, n)) return rc;
    }
    c->host_replays++;
    c->score_epoch++;        // passes in flight were scored on the device without what this replay adds
    c->exact_valid = false;
    c->rx_set_valid = c->rx_held_valid = false;
    static const bool skip_replay = tuning_env("ADSB_SKIP_REPLAY") != nullptr;  // measurement aid (tuning build only)
#ifdef ADSB_TUNING
    const auto tr0 = std::chrono::steady_clock::now();
#endif
    {
        HT(c, HT_REPLAY);
        const uint64_t before = c->filter.inserts();
        if (c->n_receivers && !skip_replay) {
            // (conservative: the address ANY receiver's filter gained may be one the union already held -- never wrong)
            bool gained = false;
            const TrialRecord *rec = sl.h_rec;
            size_t n_rec = n;
            if (sl.seam_on) {
                // the pass's own records at j < 326 tried a zero lead-in: the seam's records of these buffers take their
                // place (the replay sorts)
                merge_seam_records(sl.h_rec, n, c->seam_rec.data(), c->seam_rec.size(), chunk_offset, sl.n_chunks, (uint32_t)kLead,
                                   c->seam_merged, &c->seam_dropped, &c->seam_records);
                rec = c->seam_merged.data();
                n_rec = c->seam_merged.size();
            }
            if (int rc = replay_receivers(c, sl, rec, n_rec, chunk_offset, out, &gained)) return rc;
            if (gained) c->last_new_insert_seq = sl.scan_seq;
        } else if (!skip_replay) {
            replay(c->filter, c->crc, sl.h_rec, n, chunk_offset, out, &c->host_sorts);
        }
        if (c->filter.inserts() != before) c->last_new_insert_seq = sl.scan_seq;
    }
#ifdef ADSB_TUNING
    c->t_replay += std::chrono::duration<double>(std::chrono::steady_clock::now() - tr0).count();
#endif
    return 0;
}

// In front of a pass that collect_oldest runs again: every stream drained, so that later passes have their results on the
// host (they may have rotated the bitmaps behind an icao_flush: the caller puts the filter's addresses back) ...
static int drain_streams(adsb_ctx *c)
{
    for (hipStream_t q : c->scan_stream)
        if (q) HIP_TRY(c, hipStreamSynchronize(q));
    HIP_TRY(c, hipStreamSynchronize(c->tail_stream));
    HIP_TRY(c, hipStreamSynchronize(c->score_stream));
    return ADSB_OK;
}

// ... and a pending icao_flush kept out of the redo's sight: it belongs to the next pass submitted
struct KeepFlushPending {
    adsb_ctx *c;
    bool pending;
    explicit KeepFlushPending(adsb_ctx *ctx) : c(ctx), pending(ctx->flush_pending) { c->flush_pending = false; }
    ~KeepFlushPending() { c->flush_pending = pending; }
    KeepFlushPending(const KeepFlushPending &) = delete;
    KeepFlushPending &operator=(const KeepFlushPending &) = delete;
};

// Finish the oldest submission: replay it, or -- when a device list overflowed (far
// denser input than the lists were sized for) -- drain the stream and go chunk by
// chunk, where the worst case always fits.  Bitmap bits set by the aborted pass or by
// later passes are a harmless superset in time.
int collect_oldest(adsb_ctx *c, std::vector<adsb_msg> &out)
{
    Slot &sl = c->slot[c->collected % (uint64_t)c->n_slots];
    adsb_stats st{};
    st.n_samples = sl.n_samples;
    st.n_chunks = sl.n_chunks;
    if (sl.flush_before) flush_host_filters(c);  // icao_flush() took effect before this pass
    flush_receivers(c, sl.rx_flush);             // ... and so did the adsb_icao_flush_receiver calls recorded against it
    c->seam_taken = false;
    int rc = finish_pass(c, sl, 0, st, out);
    // whatever makes the library redo the pass's match redoes the seam's too, from scratch and independent of the
    // superset (a seam step does not depend on the pass's lists, but its match read the same bitmap)
    if (rc > 0 && sl.seam_on) {
        if (int e = drain_streams(c)) return e;
        if (int e = redo_seam(c, sl)) rc = e;
    }
    if (rc == 2) {
        // a one-launch pass that a pass in flight beside it may have invalidated (finish_pass): once more
        // through the three launches.  Passes submitted after it may have rotated the bitmaps behind an
        // icao_flush: as for the overflow fallback, drain the streams and put the filter's addresses (the
        // state that preceded this pass) back into the bitmap in use.
        c->rematches++;
        if (int e = drain_streams(c)) return e;
        const KeepFlushPending keep(c);
        PassOptions redo;   // three launches, blocking, on the input it already read
        redo.redo = redo.inline_tail = redo.no_fuse = true;
        redo.input_done = input_ready_now();
        rc = reseed_bitmap_from_filter(c);
        if (rc == 0) rc = enqueue_pass(c, sl, sl.src, sl.fmt, sl.n_samples, sl.n_chunks, redo);
        if (rc == 0) rc = finish_pass(c, sl, 0, st, out);
    }
    if (rc > 0 && sl.fmt == SrcFormat::kMag) {  // a caller-supplied buffer denser than the fast scan's lists: again, the slow way
        st.retries++;
        if (int e = drain_streams(c)) return e;
        const KeepFlushPending keep(c);
        Slot tmp;
        rc = fallback_slot(c, sl, tmp);
        if (rc == 0) rc = reseed_bitmap_from_filter(c);
        PassOptions slow;   // the reference-shaped kernel into the worst-case lists
        slow.redo = slow.force_simple = true;
        if (rc == 0) rc = enqueue_pass(c, tmp, sl.src, SrcFormat::kMag, sl.n_samples, 1, slow);
        if (rc == 0) rc = finish_pass(c, tmp, 0, st, out);
    } else if (rc > 0) {
        st.retries++;
        if (int e = drain_streams(c)) return e;
        const KeepFlushPending keep(c);
        Slot tmp;  // same counters, summary and events; one chunk at a time into the worst-case lists
        rc = fallback_slot(c, sl, tmp);
        if (rc == 0) rc = reseed_bitmap_from_filter(c);
        for (uint64_t ch = 0; ch < sl.n_chunks && rc == 0; ch++) {
            const uint64_t off = ch * kChunkSamples;
            const uint64_t n = std::min<uint64_t>(kChunkSamples, sl.n_samples - off);
            PassOptions slow;
            slow.redo = slow.force_simple = true;
            slow.lead_from_src = ch > 0;
            // (carry-over mode: buffers after the first find their lead-in in src itself; the
            // carry for the next call was already taken when the pass was first enqueued)
            // the reference-shaped kernel: its lists hold the worst case of a chunk
            if (sl.fmt == SrcFormat::kCu8) {
                // ... which reads CS16: the buffer and the lead-in it takes from src, widened into a staging buffer
                // first (in stream order in front of the pass; the pass is finished before the next buffer's turn)
                const uint64_t lead = ch > 0 ? kCarrySamples : 0;
                rc = ensure_widen(c);
                if (rc == 0)
                    if (int e = launch_widen_u8(sl.src, off - lead, (uint32_t)(n + lead), c->d_u8_table, c->d_widen, c->scan_stream[0]))
                        rc = fail(c, (hipError_t)e, "launch_widen_u8");
                if (rc == 0)
                    if (hipError_t e = hipStreamSynchronize(c->scan_stream[0])) rc = fail(c, e, "hipStreamSynchronize");
                if (rc == 0)
                    rc = enqueue_pass(c, tmp, c->d_widen + lead, SrcFormat::kCs16, n, 1, slow);
            } else {
                rc = enqueue_pass(c, tmp, (const uint32_t *)sl.src + off, SrcFormat::kCs16, n, 1, slow);
            }
            if (rc == 0) rc = finish_pass(c, tmp, ch, st, out);
        }
    }
    // (a pass the fallback or the rematch ran again launched no second k_signal_stats: the records are the first enqueue's)
    c->sig_out.clear();
    if (rc == 0 && sl.sig_on) rc = take_signal_records(c, sl);
    sl.busy = false;
    c->seam_taken = false;
    c->collected++;
    if (rc > 0) {
        c->last_error = "device lists overflowed on a single chunk";
        return ADSB_ERR_HIP;
    }
    if (rc < 0) return rc;
    c->stats = st;
    return ADSB_OK;
}

// Finish every pass in flight now; the caller still gets them from adsb_collect, in order.
int park_pending(adsb_ctx *c)
{
    std::vector<adsb_signal_stats> callers;   // (what adsb_fetch_signal_stats hands out is the caller's last collect's)
    callers.swap(c->sig_out);
    while (c->collected < c->submitted) {
        Slot &sl = c->slot[c->collected % (uint64_t)c->n_slots];
        sl.parked_msgs.clear();
        sl.park_rc = collect_oldest(c, sl.parked_msgs);
        sl.parked_stats = c->stats;
        sl.parked_sig.clear();
        sl.parked_sig.swap(c->sig_out);
        sl.parked = true;
    }
    c->sig_out.swap(callers);
    return ADSB_OK;
}

// adsb_collect: the oldest pass the caller has not had yet
int collect_next(adsb_ctx *c, std::vector<adsb_msg> &out)
{
    if (c->delivered < c->collected) {
        Slot &sl = c->slot[c->delivered % (uint64_t)c->n_slots];
        out.swap(sl.parked_msgs);
        sl.parked_msgs.clear();
        c->stats = sl.parked_stats;
        c->sig_out.swap(sl.parked_sig);
        sl.parked_sig.clear();
        sl.parked = false;
        c->delivered++;
        return sl.park_rc;
    }
    const int rc = collect_oldest(c, out);
    c->delivered++;
    return rc;
}

int deliver(adsb_ctx *c, std::vector<adsb_msg> &msgs, adsb_msg *out, size_t cap,
            size_t *n_out)
{
    c->stats.n_messages = msgs.size();
    const size_t n = std::min(cap, msgs.size());
    if (n && out) std::memcpy(out, msgs.data(), n * sizeof(adsb_msg));
    if (n_out) *n_out = msgs.size();
    c->has_undelivered = msgs.size() > cap;
    if (!c->has_undelivered) {
        c->undelivered.clear();
        return ADSB_OK;
    }
    c->undelivered.swap(msgs);  // the pass is consumed: keep what it produced (adsb_fetch_messages)
    return ADSB_ERR_CAPACITY;
}

}  // namespace host
}  // namespace adsb

extern "C" {

int adsb_collect(adsb_ctx *c, adsb_msg *out, size_t cap, size_t *n_out)
try {
    if (!c || (!out && cap)) return ADSB_ERR_INVALID;
    if (c->submitted == c->delivered) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(c);
    std::vector<adsb_msg> msgs;
    int rc = collect_next(c, msgs);
    if (rc) return rc;
    return deliver(c, msgs, out, cap, n_out);
} ADSB_ABI_CATCH

int adsb_pending(const adsb_ctx *c) { return c ? (int)(c->submitted - c->delivered) : 0; }

int adsb_fetch_messages(adsb_ctx *c, adsb_msg *out, size_t cap, size_t *n_out)
try {
    if (!c || (!out && cap) || !c->has_undelivered) return ADSB_ERR_INVALID;
    const size_t n = std::min(cap, c->undelivered.size());
    if (n) std::memcpy(out, c->undelivered.data(), n * sizeof(adsb_msg));
    if (n_out) *n_out = c->undelivered.size();
    return c->undelivered.size() > cap ? ADSB_ERR_CAPACITY : ADSB_OK;
} ADSB_ABI_CATCH

}  // extern "C"
