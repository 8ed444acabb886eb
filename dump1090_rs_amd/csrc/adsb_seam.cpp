// adsb_seam.cpp -- receiver seams (include/adsb_hip.h, "Receiver seams"): carry-over while receivers are on.  The mode,
// its storage, the two steps it adds to a pass (adsb_pass.cpp calls them), and what collect does with the seam's records
// (adsb_collect.cpp calls that).  The kernels are adsb_seam.hip's; the record merge and the previous-buffer map are host
// code of adsb_replay_host.cpp.
#include "adsb_ctx.h"
#include "adsb_seam_score_dev.h"

using namespace adsb::host;

namespace {

constexpr uint32_t kSeamRedoChunks = 8;   // buffers a redo's piece takes: 8 x 326 x 5 records, 417 KB of pinned memory

uint32_t seam_default_cap(size_t max_chunks)
{
    return (uint32_t)std::min<size_t>(std::max<size_t>(2048, 64 * max_chunks), 65536);
}

// ---- scored on the device (adsb_set_receiver_carry_scoring): the storage of the device-side merge ----
void unwire_seam_score(adsb_ctx *c)
{
    release(c, &c->d_merge_block);
    release(c, &c->h_merge_block);
    c->h_merge_block_dev = nullptr;
    for (Slot &sl : c->slot) {
        release(c, &sl.seam_matched);
        sl.seam_scored = false;
        sl.merge = SeamMergeParams{};
        sl.h_merge_sum = sl.h_merge_sum_dev = nullptr;
    }
}

// Per slot, in one device block: the merged arrays rec', si', pos', slot', flag' (52 bytes a hit, ScoreDev::cap hits), the
// mirror of the seam's record block (32 bytes a record, seam_cap records), the presence rows and the four per-buffer work
// arrays (228 bytes a buffer) and the note and state words; one 32-byte summary per slot in mapped host memory; one event
// per slot.  All or nothing, and nothing at all in a context that never scores on the device: its seam passes stay the
// host's.  Behind ensure_seam (seam_cap is set), nothing in flight.
int ensure_seam_score(adsb_ctx *c)
{
    unwire_seam_score(c);
    if (!c->score.si || !c->score.cap || !c->n_receivers) return ADSB_OK;
    const size_t cap = c->score.cap, nb = c->max_chunks;
    const size_t o_si = up256(cap * sizeof(TrialRecord)), o_pos = o_si + up256(cap * sizeof(uint32_t)),
                 o_slot = o_pos + up256(cap * sizeof(unsigned long long)), o_flag = o_slot + up256(cap * sizeof(uint32_t)),
                 o_mirror = o_flag + up256(cap * sizeof(uint32_t)), o_present = o_mirror + up256((size_t)c->seam_cap * sizeof(TrialRecord)),
                 o_start = o_present + up256(nb * kSeamKeyStride * sizeof(uint32_t)), o_drop = o_start + up256((nb + 1) * sizeof(uint32_t)),
                 o_base = o_drop + up256(nb * sizeof(uint32_t)), o_shift = o_base + up256(nb * sizeof(uint32_t)),
                 o_note = o_shift + up256(nb * sizeof(uint32_t)), o_state = o_note + 256, d_slot = o_state + up256(sizeof(SeamMergeState));
    const size_t h_slot = up256(sizeof(SeamMergeSummary));
    Rollback undo{c->mem, c->mem.mark(), false};
    HIP_TRY(c, dev_alloc(c, &c->d_merge_block, d_slot * (size_t)c->n_slots));
    HIP_TRY(c, pinned_alloc(c, &c->h_merge_block, &c->h_merge_block_dev, h_slot * (size_t)c->n_slots));
    HIP_TRY(c, hipMemset(c->d_merge_block, 0, d_slot * (size_t)c->n_slots));
    for (int si = 0; si < c->n_slots; si++) HIP_TRY(c, new_event(c, &c->slot[si].seam_matched, kQuietEvent));
    undo.keep = true;
    std::memset(c->h_merge_block, 0, h_slot * (size_t)c->n_slots);
    for (int si = 0; si < c->n_slots; si++) {
        Slot &sl = c->slot[si];
        char *d = c->d_merge_block + d_slot * (size_t)si;
        SeamMergeParams &m = sl.merge;
        m = SeamMergeParams{};
        m.merged = sl.score;   // (seam_merge copies the pass's own over it and puts these five back)
        m.merged.rec = reinterpret_cast<TrialRecord *>(d);
        m.merged.si = reinterpret_cast<uint32_t *>(d + o_si);
        m.merged.pos = reinterpret_cast<unsigned long long *>(d + o_pos);
        m.merged.slot = reinterpret_cast<uint32_t *>(d + o_slot);
        m.merged.flag = reinterpret_cast<uint32_t *>(d + o_flag);
        m.seam_rec = reinterpret_cast<TrialRecord *>(d + o_mirror);
        m.seam_cap = c->seam_cap;
        m.present = reinterpret_cast<uint32_t *>(d + o_present);
        m.own_start = reinterpret_cast<uint32_t *>(d + o_start);
        m.drop = reinterpret_cast<uint32_t *>(d + o_drop);
        m.seam_base = reinterpret_cast<uint32_t *>(d + o_base);
        m.own_shift = reinterpret_cast<uint32_t *>(d + o_shift);
        m.note = reinterpret_cast<uint32_t *>(d + o_note);
        m.st = reinterpret_cast<SeamMergeState *>(d + o_state);
        sl.h_merge_sum = reinterpret_cast<SeamMergeSummary *>(c->h_merge_block + h_slot * (size_t)si);
        sl.h_merge_sum_dev = reinterpret_cast<SeamMergeSummary *>(c->h_merge_block_dev + h_slot * (size_t)si);
        m.summary = sl.h_merge_sum_dev;
    }
    return ADSB_OK;
}

void unwire_seam(adsb_ctx *c)
{
    unwire_seam_score(c);
    release(c, &c->d_rx_carry);
    release(c, &c->h_seam_block);
    release(c, &c->d_seam_block);
    release(c, &c->seam_fb.h_rec);
    c->h_seam_block_dev = nullptr;
    c->seam_fb.h_rec_dev = nullptr;
    for (Slot &sl : c->slot) {
        sl.seam_on = false;
        sl.h_seam_desc = sl.h_seam_desc_dev = nullptr;
        sl.h_seam_sum = sl.h_seam_sum_dev = nullptr;
        sl.h_seam_rec = sl.h_seam_rec_dev = nullptr;
        sl.d_seam_ctr = nullptr;
        sl.d_seam_lead = nullptr;
        sl.d_seam_list = nullptr;
    }
}

// The mode's storage for the context's slots and c->n_receivers receivers, all or nothing; every carry starts at zero:
// nothing precedes a receiver's next buffer.  Nothing may be in flight.
int ensure_seam(adsb_ctx *c)
{
    unwire_seam(c);
    c->seam_cap = seam_default_cap(c->max_chunks);
    const size_t desc_bytes = up256(c->max_chunks * sizeof(SeamDesc)), sum_bytes = up256(sizeof(SeamSummary));
    const size_t rec_bytes = up256((size_t)c->seam_cap * sizeof(TrialRecord));
    const size_t h_slot = desc_bytes + sum_bytes + rec_bytes;
    const size_t ctr_bytes = up256(sizeof(SeamCounters)), lead_bytes = up256(c->max_chunks * (size_t)kCarrySamples * sizeof(uint32_t));
    const size_t d_slot = ctr_bytes + lead_bytes + rec_bytes;
    const size_t carry_bytes = (size_t)c->n_receivers * kCarrySamples * sizeof(uint32_t);
    Rollback undo{c->mem, c->mem.mark(), false};
    HIP_TRY(c, dev_alloc(c, &c->d_rx_carry, carry_bytes));
    HIP_TRY(c, pinned_alloc(c, &c->h_seam_block, &c->h_seam_block_dev, h_slot * (size_t)c->n_slots));
    HIP_TRY(c, dev_alloc(c, &c->d_seam_block, d_slot * (size_t)c->n_slots));
    HIP_TRY(c, hipMemset(c->d_rx_carry, 0, carry_bytes));
    HIP_TRY(c, hipMemset(c->d_seam_block, 0, d_slot * (size_t)c->n_slots));
    undo.keep = true;
    std::memset(c->h_seam_block, 0, h_slot * (size_t)c->n_slots);
    c->seam_latest.assign(c->n_receivers, -1);
    c->seam_prev.reserve(c->max_chunks), c->seam_last.reserve(c->max_chunks);
    for (int si = 0; si < c->n_slots; si++) {
        Slot &sl = c->slot[si];
        char *h = c->h_seam_block + h_slot * (size_t)si, *hd = c->h_seam_block_dev + h_slot * (size_t)si;
        char *d = c->d_seam_block + d_slot * (size_t)si;
        sl.h_seam_desc = reinterpret_cast<SeamDesc *>(h), sl.h_seam_desc_dev = reinterpret_cast<SeamDesc *>(hd);
        sl.h_seam_sum = reinterpret_cast<SeamSummary *>(h + desc_bytes);
        sl.h_seam_sum_dev = reinterpret_cast<SeamSummary *>(hd + desc_bytes);
        sl.h_seam_rec = reinterpret_cast<TrialRecord *>(h + desc_bytes + sum_bytes);
        sl.h_seam_rec_dev = reinterpret_cast<TrialRecord *>(hd + desc_bytes + sum_bytes);
        sl.d_seam_ctr = reinterpret_cast<SeamCounters *>(d);
        sl.d_seam_lead = reinterpret_cast<uint32_t *>(d + ctr_bytes);
        sl.d_seam_list = reinterpret_cast<TrialRecord *>(d + ctr_bytes + lead_bytes);
    }
    if (c->rx_carry_scoring)   // (both or neither: a seam pass scored on the device without its merge would lack the seams)
        if (int rc = ensure_seam_score(c)) {
            unwire_seam(c);
            return rc;
        }
    return ADSB_OK;
}

// the combined mode off: both single modes with it, and the storage of the seams and of the merge (the keyed sets stay
// reserved, as they do when adsb_set_receiver_scoring is switched off)
void leave_carry_scoring(adsb_ctx *c)
{
    c->rx_carry_scoring = c->rx_carry = c->rx_scoring = false;
    c->rx_set_valid = false;
    unwire_seam(c);
}

// adsb_set_receivers changed the number of receivers (nothing is in flight): none left -- the mode goes off and its
// storage with it; otherwise every receiver's stream restarts, with carries for the new number
int receivers_changed(adsb_ctx *c)
{
    if (!c->rx_carry) return ADSB_OK;
    if (!c->n_receivers) {
        if (c->rx_carry_scoring) leave_carry_scoring(c);
        c->rx_carry = false;
        unwire_seam(c);
        return ADSB_OK;
    }
    if (int rc = ensure_seam(c)) {
        if (c->rx_carry_scoring) leave_carry_scoring(c);
        c->rx_carry = false;
        return rc;
    }
    return ADSB_OK;
}

int ensure_seam_fallback(adsb_ctx *c)
{
    if (c->seam_fb.h_rec) return ADSB_OK;
    HIP_TRY(c, pinned_alloc(c, &c->seam_fb.h_rec, &c->seam_fb.h_rec_dev, (size_t)kSeamRedoChunks * kSeamWorstPerChunk * sizeof(TrialRecord)));
    return ADSB_OK;
}

uint32_t seam_cap_now(const adsb_ctx *c) { return c->seam_tune ? std::min(c->seam_tune, c->seam_cap) : c->seam_cap; }

bool seam_summary_landed(const SeamSummary *s, uint32_t seq, uint32_t w[6])
{
    if (__atomic_load_n(&s->seq, __ATOMIC_ACQUIRE) != seq) return false;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(s);
    for (int k = 0; k < 6; k++) w[k] = __atomic_load_n(&src[k], __ATOMIC_RELAXED);
    return __atomic_load_n(&s->check, __ATOMIC_RELAXED) == seam_summary_check(w, seq);
}

// the seam summary of the launches that went out with `seq`, waited for on `q`; then its n_rec records at `rec`, whole
int wait_seam(adsb_ctx *c, const SeamSummary *s, uint32_t seq, hipStream_t q, const TrialRecord *rec, uint32_t w[6])
{
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (uint32_t spin = 0; !seen; spin++) {
        seen = seam_summary_landed(s, seq, w);
        if (seen) break;
        __builtin_ia32_pause();
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    if (!seen) {
        HIP_TRY(c, hipStreamSynchronize(q));
        for (int attempt = 0; attempt < 200 && !seen; attempt++) {
            seen = seam_summary_landed(s, seq, w);
            if (!seen) for (volatile int spin = 0; spin < 2000; spin++) {}
        }
    }
    if (!seen) {
        c->last_error = "a pass's seam step completed without publishing a whole summary";
        return ADSB_ERR_HIP;
    }
    if (w[1]) return ADSB_OK;   // (overflowed: the records are redone)
    Summary sum{};
    sum.rec_sum_lo = w[2], sum.rec_sum_hi = w[3];
    return verify_records(c, &sum, rec, w[0]);
}

}  // namespace

namespace adsb {
namespace host {

int seam_front(adsb_ctx *c, Slot &sl, ScanParams &p, SrcFormat fmt, bool plain_iq, bool redo, hipStream_t ss)
{
    if (redo) {   // (a pass run again launches no second seam step: sl.seam_on stays what the first enqueue made it)
        sl.seam_scored = false;   // ... and is the host's: no merge
        return ADSB_OK;
    }
    sl.seam_on = c->rx_carry && c->n_receivers && plain_iq && sl.h_seam_desc != nullptr;
    // scored on the device (fill_pass has decided: sl.rx_scored): the pass goes through the device-side merge
    sl.seam_scored = sl.seam_on && sl.rx_scored && sl.merge.seam_rec != nullptr;
    if (!sl.seam_on) return ADSB_OK;
    if (p.bitmap_fresh) {
        // a folded bitmap behind an icao_flush is cleared by the pass's own launch -- which would wipe what the seam
        // learns in front of it: cleared here instead (stream order on `ss`; the counters the reset zeroes are zero)
        if (int e = launch_reset(sl.d_ctr, p.bitmap, p.bitmap_lg, ss)) return fail(c, (hipError_t)e, "launch_reset");
        p.bitmap_fresh = 0;
    }
    // whose buffer follows whose: the host works it out from the map (SeamDesc), into the slot's mapped descriptors
    const uint32_t n = p.n_chunks;
    c->seam_prev.resize(n), c->seam_last.resize(n);   // (within what ensure_seam reserved: no allocation per submit)
    if (sl.rx_map.size() < n || !seam_prev_map(sl.rx_map.data(), n, c->n_receivers, c->seam_latest, c->seam_prev.data(), c->seam_last.data()))
        return ADSB_ERR_INVALID;
    for (uint32_t b = 0; b < n; b++) sl.h_seam_desc[b] = SeamDesc{c->seam_prev[b], sl.rx_map[b], c->seam_last[b], 0u};
    SeamParams &q = sl.seam;
    q = SeamParams{};
    q.src = p.src;
    q.n_samples = p.n_samples;
    q.n_chunks = n;
    q.first_chunk = 0;
    q.n_scan = n;
    q.u8_table = fmt == SrcFormat::kCu8 ? c->d_u8_table : nullptr;
    q.desc = sl.h_seam_desc_dev;
    q.carry = c->d_rx_carry;
    q.n_receivers = c->n_receivers;
    q.lead = sl.d_seam_lead;
    q.bitmap = p.bitmap;
    q.bitmap_lg = p.bitmap_lg;
    q.tables = p.tables;
    q.fix = p.fix;
    q.list = sl.d_seam_list;
    q.list_cap = q.rec_cap = seam_cap_now(c);
    q.rec = sl.h_seam_rec_dev;
    q.ctr = sl.d_seam_ctr;
    q.summary = sl.h_seam_sum_dev;
    q.seq = next_seq(c);
    if (sl.seam_scored) {   // the records also into the merge's mirror, the counts into its note
        q.rec_dev = const_cast<TrialRecord *>(sl.merge.seam_rec);
        q.note = sl.merge.note;
    }
    __atomic_store_n(&sl.h_seam_sum->seq, 0u, __ATOMIC_RELEASE);   // k_seam_match overwrites it, last, with q.seq
    if (int e = launch_seam_lead(q, ss)) return fail(c, (hipError_t)e, "launch_seam_lead");
    if (int e = launch_seam_scan(q, ss)) return fail(c, (hipError_t)e, "launch_seam_scan");
    c->seam_passes++;
    return ADSB_OK;
}

int seam_tail(adsb_ctx *c, Slot &sl, hipStream_t ts)
{
    if (!sl.seam_on || sl.redo) return ADSB_OK;
    if (int e = launch_seam_match(sl.seam, ts)) return fail(c, (hipError_t)e, "launch_seam_match");
    // a three-launch pass: `recorded` says the pass is through matching against its bitmap (a later pass clears a retired
    // one behind it) -- that now includes the seam's match
    if (!sl.fused) HIP_TRY(c, hipEventRecord(sl.recorded, ts));
    // scored on the device: the merge on the score stream reads what k_seam_match has just finished (seam_merge waits)
    if (sl.seam_scored) HIP_TRY(c, hipEventRecord(sl.seam_matched, ts));
    return ADSB_OK;
}

int seam_merge(adsb_ctx *c, Slot &sl, const ScanParams &p, ScanParams *pm, hipStream_t qs)
{
    *pm = p;
    if (!sl.seam_scored) return ADSB_OK;
    SeamMergeParams &m = sl.merge;
    const ScoreDev mine = m.merged;
    m.merged = p.score;   // the pass's own: tables, state, outputs, sequence number -- with the merged arrays in place of its five
    m.merged.rec = mine.rec, m.merged.si = mine.si, m.merged.pos = mine.pos, m.merged.slot = mine.slot, m.merged.flag = mine.flag;
    m.seq = sl.seq;
    __atomic_store_n(&sl.h_merge_sum->seq, 0u, __ATOMIC_RELEASE);   // k_seam_prefix overwrites it, last, with the pass's
    HIP_TRY(c, hipStreamWaitEvent(qs, sl.seam_matched, 0));          // edge (4s)
    if (int e = launch_seam_merge(p, m, qs)) return fail(c, (hipError_t)e, "launch_seam_merge");
    pm->score = m.merged;
    return ADSB_OK;
}

void count_seam_merge(adsb_ctx *c, const Slot &sl)
{
    if (!sl.seam_scored || !sl.h_merge_sum) return;
    const SeamMergeSummary *s = sl.h_merge_sum;
    if (__atomic_load_n(&s->seq, __ATOMIC_ACQUIRE) != sl.seq) return;   // (behind the pass's `done`: it has landed)
    c->seam_sc_passes += s->merged != 0;
    c->seam_sc_records += s->n_seam;
    c->seam_sc_dropped += s->dropped;
    c->seam_sc_unscored += s->unscored != 0;
}

int take_seam(adsb_ctx *c, Slot &sl)
{
    uint32_t w[6];
    if (int rc = wait_seam(c, sl.h_seam_sum, sl.seam.seq, sl.tail_q, sl.h_seam_rec, w)) return rc;
    if (w[1]) return redo_seam(c, sl);
    c->seam_rec.assign(sl.h_seam_rec, sl.h_seam_rec + w[0]);
    c->seam_taken = true;
    return ADSB_OK;
}

// The pass's seam step once more, in pieces whose records always fit: every trial that passes the gates and has a DF
// the replay can score is a record (no list, no match: the replay scores an address/parity trial whose address its
// receiver does not know -2, as it does a false superset hit).  The lead-in rows of the first run are still in the slot.
int redo_seam(adsb_ctx *c, Slot &sl)
{
    if (int rc = ensure_seam_fallback(c)) return rc;
    hipStream_t q0 = c->scan_stream[0];
    c->seam_redone++;
    c->seam_rec.clear();
    SeamParams q = sl.seam;
    q.emit_all = 1;
    // what the seam learns goes into the bitmap in use NOW, as the overflow fallback's own scans' does: an icao_flush
    // submitted behind this pass may have rotated the bitmaps, and an address only a seam trial validates (a DF17 across
    // the buffer's start) must be in the superset the fallback's match reads, for a reply at j >= 326 of that buffer
    q.bitmap = c->d_bitmap[c->cur_bitmap];
    q.bitmap_lg = c->bitmap_lg;
    q.list = nullptr;
    q.list_cap = 0;
    q.rec = c->seam_fb.h_rec_dev;
    q.rec_cap = kSeamRedoChunks * kSeamWorstPerChunk;
    q.rec_dev = nullptr;   // (the host's from here on: the mirror holds rec_cap of the first run, and no merge follows)
    q.note = nullptr;
    for (uint32_t b0 = 0; b0 < q.n_chunks; b0 += kSeamRedoChunks) {
        q.first_chunk = b0;
        q.n_scan = std::min(kSeamRedoChunks, q.n_chunks - b0);
        q.seq = next_seq(c);
        __atomic_store_n(&sl.h_seam_sum->seq, 0u, __ATOMIC_RELEASE);
        if (int e = launch_seam_scan(q, q0)) return fail(c, (hipError_t)e, "launch_seam_scan");
        if (int e = launch_seam_match(q, q0)) return fail(c, (hipError_t)e, "launch_seam_match");
        HIP_TRY(c, hipStreamSynchronize(q0));
        uint32_t w[6];
        if (int rc = wait_seam(c, sl.h_seam_sum, q.seq, q0, c->seam_fb.h_rec, w)) return rc;
        if (w[1]) {
            c->last_error = "a seam step's worst-case record block overflowed";
            return ADSB_ERR_HIP;
        }
        c->seam_rec.insert(c->seam_rec.end(), c->seam_fb.h_rec, c->seam_fb.h_rec + w[0]);
    }
    c->seam_taken = true;
    return ADSB_OK;
}

}  // namespace host
}  // namespace adsb

extern "C" {

int adsb_set_receiver_carry(adsb_ctx *c, int enabled)
try {
    if (!c) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    // (adsb_set_receiver_carry_scoring holds both modes on: the value in effect is fine, a change is not)
    if (c->rx_carry_scoring) return enabled ? ADSB_OK : ADSB_ERR_INVALID;
    // (seam trials are scored by the host: not together with adsb_set_receiver_scoring)
    if (!c->n_receivers || c->rx_scoring) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(c);
    if (enabled) {
        // every receiver's stream starts here, with nothing before its next buffer
        c->seam_receivers_changed = receivers_changed;
        if (int rc = ensure_seam(c)) {
            c->rx_carry = false;
            return rc;
        }
        c->rx_carry = true;
    } else if (c->rx_carry) {
        c->rx_carry = false;
        unwire_seam(c);
    }
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_get_receiver_carry(const adsb_ctx *c) { return c ? (c->rx_carry ? 1 : 0) : ADSB_ERR_INVALID; }

int adsb_set_receiver_carry_scoring(adsb_ctx *c, int enabled)
try {
    if (!c) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered || c->shard_active) return ADSB_ERR_BUSY;
    if (!c->n_receivers) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(c);
    if (!enabled) {
        if (c->rx_carry_scoring) leave_carry_scoring(c);
        return ADSB_OK;
    }
    // from any state of the two single modes: what both reserve, then the merge's own; every receiver's stream restarts
    c->seam_receivers_changed = receivers_changed;
    c->rx_carry_scoring = c->rx_carry = c->rx_scoring = true;
    c->rx_set_valid = false;   // (the next scored pass rebuilds what it scores against)
    int rc = ensure_rx_scoring(c);
    if (rc == ADSB_OK) rc = ensure_seam(c);
    if (rc != ADSB_OK) leave_carry_scoring(c);
    return rc;
} ADSB_ABI_CATCH

int adsb_get_receiver_carry_scoring(const adsb_ctx *c) { return c ? (c->rx_carry_scoring ? 1 : 0) : ADSB_ERR_INVALID; }

int adsb_selftest_rx_seam_score_counters(const adsb_ctx *c, uint64_t *out4)
{
    if (!c || !out4) return ADSB_ERR_INVALID;
    out4[0] = c->seam_sc_passes, out4[1] = c->seam_sc_records, out4[2] = c->seam_sc_dropped, out4[3] = c->seam_sc_unscored;
    return ADSB_OK;
}

int adsb_receiver_carry_reset(adsb_ctx *c, uint32_t receiver)
try {
    if (!c || !c->rx_carry || (receiver != ADSB_RX_ALL && receiver >= c->n_receivers)) return ADSB_ERR_INVALID;
    ADSB_ON_DEVICE(c);
    // in stream order between the seam steps of the passes submitted before and after it: they all run on the first scan stream
    const size_t row = (size_t)kCarrySamples * sizeof(uint32_t);
    if (receiver == ADSB_RX_ALL) HIP_TRY(c, hipMemsetAsync(c->d_rx_carry, 0, row * c->n_receivers, c->scan_stream[0]));
    else HIP_TRY(c, hipMemsetAsync(c->d_rx_carry + (size_t)receiver * kCarrySamples, 0, row, c->scan_stream[0]));
    return ADSB_OK;
} ADSB_ABI_CATCH

int adsb_selftest_rx_seam_tune(adsb_ctx *c, uint32_t list_cap)
{
    if (!c) return ADSB_ERR_INVALID;
    if (c->submitted != c->delivered) return ADSB_ERR_BUSY;
    c->seam_tune = list_cap;
    return ADSB_OK;
}

int adsb_selftest_rx_seam_counters(const adsb_ctx *c, uint64_t *out4)
{
    if (!c || !out4) return ADSB_ERR_INVALID;
    out4[0] = c->seam_passes, out4[1] = c->seam_records, out4[2] = c->seam_dropped, out4[3] = c->seam_redone;
    return ADSB_OK;
}

}  // extern "C"
