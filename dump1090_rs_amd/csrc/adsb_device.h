// adsb_device.h -- data that crosses the kernel/host line inside libadsb_hip.so.
//
// Device pipeline for one call over C chunks (chunk = one MagnitudeBuffer's worth of
// samples, 131072, reference src/lib.rs:22):
//
//   scan    IQ -> per-tile magnitudes in LDS -> sign planes -> preamble pattern
//           (bit-parallel) -> SNR/quiet gates -> 5 trial phases per candidate: DF + CRC-24
//           syndrome straight from the sign planes ->
//             * self-validating trials (clean DF11 / DF17 / DF18)  -> hit list,
//               and their address is OR-ed into the 2^24-bit address bitmap
//             * address/parity trials (DF 0,4,5,16,20,21,24..31)   -> AP list
//   match   AP list x bitmap -> hit list      (bitmap is now complete for the call)
//   records hit list -> {chunk, j, try_phase, 14 message bytes, 33-sample power}
//
// The host then replays the records in (chunk, j, try_phase) order through the
// reference's score/filter logic.  Trials the device drops can neither add to the
// filter nor score >= 0, so the replay is exact ("Why the split is exact").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "adsb_record.h"
#include "adsb_tables.h"

// Measurement switches (tools/*.sh: ADSB_DEBUG_STOP, ADSB_STAGGER, ADSB_SCAN_BLOCKS_PER_CU,
// ADSB_STREAM_PRIO, ADSB_NO_EXT_EVENTS, ADSB_ONE_SCAN_STREAM, ADSB_DONE_FENCE, ADSB_TIMELINE) exist
// only in a library built with -DADSB_TUNING (-DADSB_KERNEL_ACCT implies it): the release build
// reads nothing from the environment, so no stray variable can change what it computes.
#if defined(ADSB_KERNEL_ACCT) && !defined(ADSB_TUNING)
#define ADSB_TUNING 1
#endif
#ifdef ADSB_TUNING
#define ADSB_STOP_AT(p, n) ((p).debug_stop == (n))
#else
#define ADSB_STOP_AT(p, n) false
#endif

namespace adsb {

inline const char *tuning_env(const char *name)
{
#ifdef ADSB_TUNING
    return std::getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

constexpr int kChunkSamples = 131072;  // MODES_MAG_BUF_SAMPLES, src/lib.rs:22
constexpr int kLead = 326;             // TRAILING_SAMPLES, src/lib.rs:24
constexpr int kMagDataLen = kLead + kChunkSamples;
constexpr int kReach = 290;            // furthest sample a preamble at j touches: j+290

// 64-bit list entry: value24 | code<<24 | j<<28 | chunk<<45
//   code 0..4   short message (56 bits), try_phase = 4 + code, value = H' (see below)
//   code 5..9   long message (112 bits), try_phase = 4 + code - 5, value = H'
//   code 10..14 try_phase = 4 + code - 10, value = the CRC residual itself
// H' = x^51 * H is the CRC syndrome of the fast scan: the residual itself for a 56-bit
// message, and the residual is x^56 * H' in GF(2)[x]/(0x1FFF409) for a 112-bit one -- the
// match kernel applies that multiplier (adsb_tables.h explains the factorisation).
__host__ __device__ inline uint64_t pack_entry(uint32_t value, uint32_t code, uint32_t j,
                                               uint64_t chunk)
{
    return (uint64_t)(value & 0xFFFFFFu) | ((uint64_t)code << 24) | ((uint64_t)j << 28) |
           (chunk << 45);
}
__host__ __device__ inline uint32_t entry_value(uint64_t e) { return (uint32_t)e & 0xFFFFFFu; }
__host__ __device__ inline uint32_t entry_code(uint64_t e) { return (uint32_t)(e >> 24) & 15u; }
__host__ __device__ inline uint32_t entry_tp(uint64_t e) { return 4u + entry_code(e) % 5u; }
__host__ __device__ inline uint32_t entry_j(uint64_t e) { return (uint32_t)(e >> 28) & 0x1FFFFu; }
__host__ __device__ inline uint64_t entry_chunk(uint64_t e) { return e >> 45; }
constexpr uint64_t kMaxChunks = 1ull << 19;  // per device pass (256 GiB of IQ)


// The AP list of the fast scan is split into kApWaveSegs equal segments: every wave of
// every persistent workgroup owns one outright, so appending needs no atomic and no shared
// counter at all (a returning global atomic costs a workgroup 1-2 us per tile, one hot
// counter saturates near 90 atomics/us on this chip, and even an LDS counter is a round
// trip per trial pass).  The simple kernel appends to a second list, `dap`, through one
// shared counter: it is the slow path anyway.
constexpr int kHitFieldWords = 8;  // ScanParams::hit_fields: f0..f4, flag, 2 spare
constexpr int kNewAddrCap = 16;
constexpr int kFusedMaxTiles = 16 * 18;  // the largest one-launch pass: 16 buffers of 17 tiles (18 with -DADSB_TILE=7284)
constexpr int kApSegments = 1280;
constexpr int kApWaveSegs = 4 * kApSegments;  // one per wave of a persistent workgroup

// Device counters block (one per context).
struct Counters {
    uint32_t n_hits;       // entries in the hit list
    uint32_t overflow;     // bit0: hit list, bit1: an AP segment, bit3: dap list
    uint32_t scan_blocks_done;  // one-launch pass: scan workgroups that have finished (the last one runs the tail)
    uint32_t n_dap;        // entries in the dap list
    uint32_t n_cand_simple;  // candidates seen by the simple kernel (diagnostic)
    uint32_t blocks_done;    // records kernel: blocks that have finished (last one publishes)
    uint32_t rec_sum[2];     // records kernel: 64-bit sum of every u64 word of the records it wrote (8-byte aligned)
    uint32_t learned_new;    // one-launch pass: how often a trial of this pass set an address bit that was clear before
    uint32_t n_rec;          // one-launch pass: records its workgroups have written in place (k_scan_fast: emit_records)
    uint32_t new_addr[kNewAddrCap];  // ... and the first of those addresses
    uint32_t unordered;      // one-launch pass: a workgroup gave up waiting for the tiles before its own (bounded wait)
    uint32_t t_start[2];     // one-launch pass: the 100 MHz wall clock when its first workgroup started
    uint32_t bitmap_ready;   // one-launch pass behind an icao_flush: its first workgroup has cleared the (folded) bitmap
    uint32_t n_fresh;        // shard phase 1 (ScanParams::fresh): distinct addresses this scan's trials can add ...
    uint32_t fresh_sum;      // ... and the sum of those addresses (the host checks the list it reads against it)
    uint32_t tile_done[kFusedMaxTiles];  // one-launch pass: tile t's address bits and list entries are published
    uint32_t seg_ap[kApWaveSegs];    // entries in each wave's AP segment
    uint32_t seg_cand[kApSegments];  // candidates seen by each fast workgroup (diagnostic)
};

// What the host needs after a pass, gathered by the records kernel (the last one to run)
// so that one small copy brings it back.
struct Summary {
    uint32_t n_hits, overflow;
    uint32_t rec_sum_lo;    // 64-bit sum of every u64 word of the n_hits records (low half): the records and
                            // this summary reach host memory as separate posted writes -- a record that has
                            // not landed (or is torn) when the host reads it makes the sums disagree
    uint32_t n_dap;
    uint32_t n_ap_total;    // all AP entries (fast segments + dap)
    uint32_t n_cand_total;  // all candidates
    uint32_t rec_sum_hi;
    uint32_t seq;           // the pass's sequence number (never 0): lets the host check it reads its own pass
    uint32_t ticks;         // one-launch pass: its duration on the device's 100 MHz wall clock, first workgroup's
                            // entry to the summary (written before seq): the launch needs no timing events
    uint32_t check;         // summary_check() of the nine words above: the ten words are separate posted writes,
                            // and a host that polls `seq` must not pair it with a neighbour that has not landed
};

// The summary's own checksum: each word rotated by its index (a swap of two words changes it), folded.
__host__ __device__ inline uint32_t summary_check(const uint32_t w[9])
{
    uint32_t x = 0xA5D5B17Cu;
    for (int k = 0; k < 9; k++) x ^= (w[k] << (k + 1)) | (w[k] >> (31 - k));
    return x;
}

// GF(2) tables, 256 u32 each (adsb_tables.h): F'0 F'1 F'2 | X56_0..2
constexpr int kTabF = 0, kTabX56 = 3, kTabCount = 6;
// after them in the same buffer: R16 (16 u32, adsb_tables.h) and the field table (300 u32)
constexpr int kTabR16Off = kTabCount * 256, kTabFieldOff = kTabR16Off + 16, kTabBitsOff = kTabFieldOff + 300,
              kTabFixOff = kTabBitsOff + 168,  // + per-bit residual constants (build_bit_residuals)
              // + the single-bit repair table and its multiplier (build_fix_table), then the two-bit table, 16-byte aligned
              kTabFix2Off = (kTabFixOff + kFixSlots + 1 + 3) & ~3,
              kTabWords = kTabFix2Off + kFix2Words;  // (build_fix2_table: its multipliers, then its buckets)

// Device-side scoring of a pass whose hits are in (buffer, j, try_phase) order: the sequential part
// of demodulate2400 (src/mode_s/mod.rs:34-139 scores read AND write the ICAO filter,
// src/demod_2400.rs:184-207 keeps the best of the five phases) done in parallel.  What makes that
// possible: a trial's score depends on the filter only through "is value v in the filter when this
// trial is scored", and v is in it then iff it was in it when the pass began (the exact bitmap) or an
// EARLIER trial of the pass added it -- the first index at which a clean DF11 (IID 0) / DF17 with
// address v occurs, found with one atomic-min hash table over the adders.  (DF18 adds addr | 1 << 25,
// which no 24-bit test value equals.)  The only thing this cannot reproduce is the reference's
// behaviour once the 4096-slot table fills up; the host checks the count and replays such a pass
// itself from the records, which are always there.
struct ScoreState {
    uint32_t n;            // hits of this pass (0 when it is not to be scored: overflow, too many)
    uint32_t blocks_done;  // k_emit
    uint32_t scored;       // 1: k_score / k_emit handle this pass (a pass without a single hit included)
    uint32_t reserved;     // a receivers pass (adsb_score_rx.hip): an insertion ran out of probes; k_emit_rx zeroes it again
    unsigned long long msg_sum;  // 64-bit sum of every u64 word of the messages written
};
struct ScoreSummary {      // in mapped host memory
    uint32_t n_msgs, n_adds;
    uint32_t msg_sum_lo, msg_sum_hi;
    uint32_t scored;       // 1: messages / adds are the pass's result; 0: the host replays the records
    uint32_t no_room;      // a receivers pass (k_emit_rx): an insertion into a keyed table ran out of probes (then scored = 0)
    uint32_t pad;
    uint32_t seq;
};
struct ScoreDev {
    uint32_t cap;                  // hits a pass may have to be scored here
    uint32_t *si;                  // per hit: value24 | kind << 24
    TrialRecord *rec;              // per hit: the record (device copy)
    unsigned long long *pos;       // per hit: buffer << 24 | j (what groups the five trial phases of a position)
    uint32_t *flag;                // per hit: bit 0 emit, bit 1 add; bits 8..18: score + 3; a repaired trial's flipped bits:
                                   // b in bits 25..31, a in bits 19..24 and bit 2 (adsb_aux.hip: k_score)
    unsigned long long *hash;      // adders: (value << 32 | first index), ~0 = empty
    uint32_t hash_mask;
    uint32_t *slot;                // per hit: the hash slot its key sits in (adders), else 0xFFFFFFFF
    uint32_t *blk;                 // per k_score block: emits, adds
    uint32_t *exact;               // 2^24 bits: the filter as it stands before this pass
    const uint32_t *earlier;       // a shard of an adsb_multi: 2^24 bits, the addresses the shards BEFORE this one (lower
                                   // buffer ranges of the same capture) add to the filter -- in it for every trial of this
                                   // shard, whichever adds them first over there; null everywhere else
    uint32_t *exact_retired;       // after an icao_flush: the bitmap the passes before it used, for k_emit to
                                   // clear (the next flush switches back to it), else null
    ScoreState *state;
    void *out_msgs;                // adsb_msg[cap], mapped host memory
    uint32_t *out_adds;            // mapped host memory: values handed to icao_filter_add, in order
    ScoreSummary *summary;         // mapped host memory
    uint32_t seq;
};
// ScoreDev::hash: where the probes of value v start (masked with hash_mask by whoever probes: score_hash_insert in
// adsb_tail_dev.h, score_hash_first in adsb_aux.hip), and how many slots a context whose passes score up to `cap` hits
// gets -- the smallest power of two >= 2 cap, so the table is at most half full and the unbounded probe loops end.
__host__ __device__ inline uint32_t score_hash_slot(uint32_t v) { return (v * 2654435761u) >> 8; }
inline uint32_t score_hash_size(uint32_t cap)
{
    uint32_t hsize = 1;
    while (hsize < 2 * cap) hsize <<= 1;
    return hsize;
}
constexpr int kScoreBlocks = 256;  // k_score / k_emit grid: block b owns a contiguous run of hits
enum ScoreKind : uint32_t { kSkOther = 0, kSkApShort, kSkApLong, kSkDf11Iid0, kSkDf11, kSkDf17, kSkDf18, kSkNone };

// Device-side scoring with one filter per receiver (adsb_set_receiver_scoring; adsb_score_rx.hip).  The argument of
// ScoreDev with one change of key: "v is in the filter of THIS BUFFER'S RECEIVER r when trial i is scored" iff (r, v) was
// in r's filter when the pass began -- the keyed exact set -- or an earlier trial of the pass in one of r's buffers added
// it -- the keyed first-adder table.  Key = r << 24 | v (r < 16384: 38 bits).  Both tables are open addressing over
// 64-bit words, ~0 = empty, nothing is ever deleted, and BOTH probe loops stop after a constant number of slots: an
// insertion that finds neither its key nor an empty slot by then sets ScoreState::reserved, the pass's summary says
// scored = 0 and the host replays the records; a lookup may stop there too, because a key that is in the table sits
// within that many slots of its home.  Parameters of their own beside ScanParams: the plain kernels see the layout they
// always had.
constexpr uint32_t kRxSetLgMin = 13, kRxSetLgMax = 22;   // slots of a keyed set: 2^13 (64 KB) .. 2^22 (32 MiB)
constexpr uint32_t kRxProbeMax = 64;                    // slots an insertion or a lookup walks at most
__host__ __device__ inline uint32_t rx_set_home(unsigned long long key, uint32_t lg)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64u - lg));   // Fibonacci hashing: the top lg bits (1 <= lg <= 32)
}
struct ScanParams;
struct RxScoreDev {
    const uint32_t *rx_map;        // the receiver of every buffer of the pass (n_chunks; buffer = pos >> 24)
    unsigned long long *first;     // adders: key << 24 | first index (i < 2^24), the size of ScoreDev::hash
    uint32_t first_lg;
    uint32_t *rx_slot;             // per hit: the slot of `first` its key sits in (adders), else 0xFFFFFFFF
    uint32_t *out_add_rx;          // mapped host memory, beside ScoreDev::out_adds: the receiver of every addition
    unsigned long long *set;       // the keyed exact set: the filters as they stand before this pass
    uint32_t set_lg, probe_max;
    unsigned long long *set_retired;   // after an icao_flush: the set the passes before it used, for k_emit_rx to clear
    uint32_t retired_lg;
};
// k_rx_adders, k_score_rx, k_emit_rx on `stream`, in that order
int launch_score_rx(const ScanParams &p, const RxScoreDev &x, void *stream);
// insert n keys into a keyed set; *d_failed += insertions that ran out of probes
int launch_rx_set_fill(const unsigned long long *d_keys, uint32_t n, unsigned long long *set, uint32_t set_lg, uint32_t probe_max,
                       uint32_t *d_failed, void *stream);
// self-test: out[i] = 1 when queries[i] is found by the lookup k_score_rx uses
int launch_rx_set_lookup(const unsigned long long *d_queries, uint32_t n, const unsigned long long *set, uint32_t set_lg,
                         uint32_t probe_max, uint32_t *d_out, void *stream);

struct ScanParams {
    const void *src;        // IQ as {re,im} int16 pairs, or u16 magnitudes (from_mag)
    uint64_t n_samples;     // IQ: total samples in the call.  from_mag: `length` of the buffer
    uint32_t n_chunks;
    uint32_t *bitmap;       // 2^bitmap_lg bits + the 4096-bit summary
    uint32_t bitmap_lg;     // 24: bit a is address a; kSmallBitmapLg: folded (contexts for passes of a few buffers)
    uint32_t bitmap_fresh;  // an icao_flush precedes this pass and `bitmap` is the next one in the rotation, NOT yet
                            // clean: a one-launch pass clears it itself -- its first workgroup does, the others wait for
                            // Counters::bitmap_ready before they touch it (folded bitmaps only: 64 KB); every pass that
                            // used it has been collected (one bitmap more than passes in flight), so nobody is waited for
    uint64_t *hits;
    uint32_t hits_cap;
    uint64_t *ap;           // wave segment g at ap + g * seg_cap (only the segments a context's largest pass can use are allocated)
    uint32_t ap_cap;        // entries allocated
    uint32_t seg_cap;       // entries per wave segment
    uint64_t *dap;          // AP entries of the simple kernel
    uint32_t dap_cap;
    const uint32_t *tables; // kTabCount x 256
    Counters *ctr;
    uint32_t *clean_bitmap; // a retired bitmap for the records kernel to clear (after an icao_flush), or null
    Summary *summary;       // in mapped host memory
    uint32_t seq;           // this pass's sequence number
    void *ev_start, *ev_stop;  // HIP events stamped by the scan launch itself (or null)
    uint32_t stagger_ticks; // fast scan: start offset between the workgroups of a CU (clock64 ticks)
    int debug_stop;         // profiling only (ADSB_DEBUG_STOP): leave the fast scan after phase N
    unsigned long long *timeline;  // profiling only (ADSB_TIMELINE): per-phase clock stamps, or null
    uint32_t keep_counters; // records kernel: leave the counters and lists as they are (first phase of a shard)
    // first phase of a shard of an adsb_multi: every address a trial of this scan can add to the filter is appended
    // here (mapped host memory), once -- fresh_seen, 2^24 bits of the shard's own, all clear when the scan starts, says
    // which have been.  That list is all the exchange needs: no records kernel and no per-record work on the host in
    // the first phase.  (Not "whose bit in `bitmap` was clear": the scans of consecutive captures overlap on two
    // streams, and the later one may set an address's bit first -- the earlier capture's list would then lack an address
    // its own second phase on the OTHER devices needs; found by the soak, tests/fuzz_gpu.py --multi.)  Null elsewhere.
    uint32_t *fresh;
    uint32_t fresh_cap;
    uint32_t *fresh_seen;
    // carry-over mode (opt-in, not the reference's semantics): the 326-sample lead-in of a
    // buffer holds the samples that preceded it.  Buffers after the first take them from src
    // itself; the first takes them from `carry` (kCarrySamples IQ samples, the end of the
    // previous call), or from src[-kCarrySamples..] when lead_from_src is set.
    const uint32_t *carry;
    uint32_t lead_from_src;
    // device-side ordering of the hit list (k_order_prefix / k_records; null: the host sorts).
    // Whoever finds a hit puts it straight into its buffer's bucket, in the sub-bucket of its tile --
    // order_tmp[chunk * kOrderBucket + tile * kTileBucket + place] -- and the hit list proper is written by k_records,
    // each buffer's bucket sorted, at the buckets' exclusive prefix (order_base, one per buffer).  order_cnt: one count
    // per TILE (17 n_chunks), all zero between passes; order_base: n_chunks + 1; order_tmp: n_chunks * kOrderBucket.
    uint32_t *order_cnt, *order_base;
    uint64_t *order_tmp;
    // self-test only (adsb_selftest_stage_lists): every position that passes the gates is also
    // appended here as chunk << 32 | j; null in every production pass
    uint64_t *cand_out;
    uint32_t *cand_count;
    uint32_t cand_cap;
    // device-side scoring (k_score / k_emit; score.si null: the host replays the records)
    ScoreDev score;
    // What the scan already knows about a self-validating hit, handed to the record builder: per slot of the
    // hit list (p.hits index, or buffer * kOrderBucket + place in the bucket) eight words -- the five bit-class
    // fields of the trial (message bit 5k + r = bit k of field r: all 112 sliced bits) and a flag that says
    // they are there.  Hits the match finds (address/parity trials) clear the flag: their message is sliced
    // from the samples as before.  Null: nobody writes or reads it.
    uint32_t *hit_fields;
    // one-launch pass (k_scan_fast<.., FUSED>: scan + match + records in one kernel, for passes of a few
    // buffers): where its records go (mapped host memory), else null
    TrialRecord *fused_rec;
    // ... a host-pointer call copies its samples into pinned memory WHILE the launch is on its way: how many
    // samples of src are there so far (a word in mapped host memory the copying thread advances; null: all)
    const unsigned long long *src_ready;
    uint32_t src_host;      // one-launch pass: `src` is host memory read in place over the link (its tiles trickle in)
    uint32_t order_polls;   // ... how often a workgroup polls for the tiles before its own before it gives up
                            // (200, ~0.2 ms; the self-test hook sets 0: every tile gives up, the second look decides)
    // CU8 passes (the U8 instantiations): `src` holds 2 bytes per sample, widened through this int16_t[256] table
    // in device memory (adsb_set_u8_table).  Last, so that the CS16 instantiations see the layout they always had.
    const uint16_t *u8_table;
    // the pass's error-correction mode (adsb_set_error_correction: 0, 1 or 3).  Non-zero: its scan is a fix instantiation
    // (k_scan_fix / k_scan_fix2, k_scan_simple<.., true> / k_scan_simple_fix2), whose DF17/18 trials with a repairable
    // residual are hits, and k_score / k_emit score and repair those (adsb_fix_dev.h).  After everything else.
    uint32_t fix;
};



// The address bitmap: 2^24 bits, followed by a 4096-bit summary (bit a & 4095 is set when any
// address a is): the match kernel tests the summary from LDS and goes to the big bitmap only
// for the few per cent of residuals that pass it.
constexpr uint32_t kBitmapWords = 1u << 19, kCoarseWords = 128;
constexpr uint32_t kBitmapAllocWords = kBitmapWords + kCoarseWords;
// A context for passes of a few buffers keeps its supersets FOLDED: 2^19 bits (64 KB) addressed by a ^ (a >> 19)
// instead of 2^24 (2 MiB) addressed by a.  The bitmap only has to be a superset of the filter (DESIGN.md section 3:
// a false positive costs one more trial record, which the ordered replay scores against the real filter), a receiver
// hears a few hundred aircraft, and such a context used to carry eleven 2 MiB bitmaps -- 23 of its 33 MB -- and clear
// one behind every icao_flush.  bitmap_lg = log2 of the bits: 24 (exact) or kSmallBitmapLg.
constexpr uint32_t kFullBitmapLg = 24, kSmallBitmapLg = 19;
__host__ __device__ inline uint32_t bitmap_words(uint32_t lg) { return 1u << (lg - 5u); }
__host__ __device__ inline uint32_t bitmap_alloc_words(uint32_t lg) { return bitmap_words(lg) + kCoarseWords; }
__host__ __device__ inline uint32_t bitmap_index(uint32_t a, uint32_t lg)
{
    return lg >= kFullBitmapLg ? a : ((a ^ (a >> lg)) & ((1u << lg) - 1u));
}

// hits one buffer's bucket holds on a dense stream (device-side ordering): ~20x a busy airspace;
// a fuller one is an overflow like any other list's (the pass is redone buffer by buffer)
constexpr uint32_t kOrderBucket = 1024;
// ... cut into one sub-bucket per tile of the buffer (17 of them): a tile has ONE writer in the scan, so its staged
// hits go to places 0 .. n-1 of its sub-bucket and its count is a plain store -- no returning atomic, no wait, no
// barrier at the end of a tile (round 5: the two dependent atomics there, behind an s_waitcnt that also covered the
// next tile's prefetch, were the dense stream's 13 us; profiles/r5_dense_acct.txt).  order_cnt has one count per tile.
constexpr uint32_t kTileBucket = 56;   // (x 18 tiles <= kOrderBucket, should the tile ever shrink: adsb_scan_geometry.h)
constexpr int kCarrySamples = 328;  // kLead rounded up to whole 16-byte loads

// What a pass's `src` holds: caller-supplied magnitudes (adsb_demodulate2400), CS16 IQ ({re, im} int16 pairs) or
// CU8 IQ ({re, im} bytes, widened through ScanParams::u8_table).  Each is its own kernel instantiation.
enum class SrcFormat : uint8_t { kMag, kCs16, kCu8 };
inline uint32_t src_bytes_per_sample(SrcFormat f) { return f == SrcFormat::kCu8 ? 2u : 4u; }

// launches; all asynchronous on `stream`, return a hipError_t as int
// (u8_table: the CU8 widening table, device memory; null for CS16 input)
int launch_to_mag(const void *d_iq, uint32_t n, uint16_t *d_data, void *stream, const uint16_t *u8_table = nullptr);
// CU8 samples [first, first + count) of d_src widened into CS16 dwords at dst (the overflow fallback's staging)
int launch_widen_u8(const void *d_src, uint64_t first, uint32_t count, const uint16_t *u8_table, uint32_t *dst, void *stream);
// zero a counters block and, when `bitmap` is non-null, clear an address bitmap (bit 0 stays
// set); only needed once per context: afterwards every pass cleans up for the next one
int launch_reset(Counters *ctr, uint32_t *bitmap, uint32_t bitmap_lg, void *stream);
// fast (IQ) or simple (mag).  sparse_ok: the caller lets a pass that uses none of the scan's optional features (the sparse
// stream of a large context: adsb_scan_fast.hip, sparse_scan_eligible) run k_scan_sparse, the same scan with those
// features folded out; *ran_sparse says whether this launch did
int launch_scan(const ScanParams &p, SrcFormat fmt, void *stream, bool sparse_ok = false, bool *ran_sparse = nullptr);
// the whole pass in one launch (p.fused_rec set): one workgroup per tile, the last one to finish matches
// what the pass learned late, builds the records and publishes the summary; for passes of a few buffers
int launch_pass_fused(const ScanParams &p, SrcFormat fmt, void *stream);
int scan_resident_blocks();  // workgroups of the fast scan's persistent grid (<= kApSegments)
int launch_scan_simple(const ScanParams &p, SrcFormat fmt, void *stream);  // reference-shaped path (not CU8: launch_widen_u8 first)
// sparse_fast: the pass is a large context's host-ordered three-launch pass behind the fast scan (adsb_pass.cpp:
// enqueue_tail) -- its match is k_match_sparse and its records kernel a small fixed grid; every other caller's stay as they are
int launch_match(const ScanParams &p, void *stream, bool sparse_fast = false);
int launch_records(const ScanParams &p, SrcFormat fmt, TrialRecord *d_rec, void *stream, bool sparse_fast = false);
// sort the hit list by (buffer, j, try_phase) on the device, so that the records come out in the
// order the host replays them in (src/demod_2400.rs:121,158: ascending j, then try_phase)
int launch_order_hits(const ScanParams &p, void *stream);
// first phase of a shard that lists its fresh addresses (ScanParams::fresh): the summary alone -- n_hits, overflow,
// Summary::rec_sum_lo = sum of the fresh addresses, Summary::n_dap = how many -- behind the scan on its stream
int launch_shard_summary(const ScanParams &p, void *stream);
// score the (ordered) hits of the pass on the device: messages, filter additions and a summary
// into mapped host memory (p.score)
int launch_score(const ScanParams &p, void *stream);
// OR a list of 24-bit addresses into a bitmap (addresses learned by other shards)
int launch_set_addresses(const uint32_t *d_addrs, uint32_t n, uint32_t *bitmap, uint32_t bitmap_lg, void *stream);
// next[i] = sample (n - kCarrySamples + i) of the stream: from d_src, or from `prev` where the
// call was shorter than the carry.  The carry is always CS16: CU8 input (u8_table set) is widened into it
int launch_update_carry(const uint32_t *prev, const void *d_src, uint64_t n_samples, uint32_t *next, void *stream,
                        const uint16_t *u8_table = nullptr);
int launch_mag_digest(uint32_t first_bits, uint32_t count, unsigned long long *d_out, void *stream);

// Signal statistics (adsb_set_signal_stats; adsb_stats.hip: k_signal_stats): one adsb_signal_stats per buffer of a
// pass.  A kernel of its own beside the scan, with parameters of its own -- ScanParams and the scan's instantiations
// stay as they are.
constexpr int kSigHistBins = 60;
constexpr int kSigRecordWords = 68;      // sizeof(adsb_signal_stats) / 4
constexpr int kSigMaxWgPerChunk = 64;    // workgroups a buffer is cut into at most (a power of two)
struct SigParams {
    const void *src;          // the pass's IQ: CS16 dwords or CU8 byte pairs, 16-byte aligned
    uint64_t n_samples;
    uint32_t n_chunks;
    uint32_t wg_per_chunk;    // signal_stats_wg_per_chunk(n_chunks)
    const uint16_t *u8_table; // CU8: the widening table (device memory), else null
    uint32_t *partial;        // device memory, kSigRecordWords per buffer, laid out as the record: all zero between passes
    uint32_t *ticket;         // device memory, one per buffer: workgroups of the buffer that have finished; zero between passes
    void *records;            // mapped host memory: adsb_signal_stats[n_chunks], each written once by its buffer's last workgroup
};
uint32_t signal_stats_wg_per_chunk(uint32_t n_chunks);
int launch_signal_stats(const SigParams &p, SrcFormat fmt, void *stream);
// Frequency shift (adsb_mix_*; adsb_mix_dev.h): the table a decimator or resampler mixes its input with on the way
// in, as the MIX instantiations of its kernels read it.  k_mix_store (adsb_decim.hip) writes the table from its kernel
// arguments: ordered on the stream, and the caller's table is copied when the launch returns.
constexpr uint32_t kMixMaxPeriod = 256;
struct MixParams {
    const uint2 *table;         // device memory, [period]: .x = {c, -s}, .y = {s, c} as int16 pairs; null: no mixer
    uint32_t period;            // N, 1 .. 256 (0: no mixer)
    uint32_t phase;             // P mod N: the table entry of the call's first input
    uint32_t recip;             // ceil(2^32 / N) (unused where N is 1)
};
struct MixTable { uint32_t cs[kMixMaxPeriod]; };   // {c, s} as int16 pairs, c in the low half
bool mix_params_ok(const MixParams &m);
int launch_mix_store(const MixTable &t, uint32_t period, uint2 *d_table, void *stream);
// Sample formats (adsb_fmt_*; include/adsb_hip.h, "Sample formats"): what a decimator's or resampler's `src` holds, the
// values of ADSB_DECIM_CS16, _8BIT, _CF32 and _REAL16.  Each is its own instantiation of the four kernels; the format
// fixes the bytes of a sample -- hence the samples of a 16-byte load -- and the conversion to CS16 in front of the mixer.
enum InFormat : uint32_t { kInCs16 = 0, kIn8Bit = 1, kInCf32 = 2, kInReal16 = 3, kInFormats = 4 };
__host__ __device__ constexpr uint32_t in_bytes_per_sample(uint32_t f) { return f == kInCf32 ? 8u : f == kInCs16 ? 4u : 2u; }
constexpr float kInDefaultScale = 32768.0f, kInMaxScale = 2147483648.0f;   // CF32: 0 < g <= 2^31
// what a launch checks: a format there is, the 8-bit table exactly where the format reads it, CF32's scale in range
bool in_format_ok(uint32_t format, const uint16_t *u8_table, float scale);
// Decimation (adsb_decim_*; adsb_decim.hip: k_decim, k_decim_history): one call's inputs -> its outputs and the
// history the next call starts from.  A kernel of its own in front of the scan, with parameters of its own.
constexpr uint32_t kDecimTile = 256;        // outputs per workgroup
constexpr uint32_t kDecimMinFactor = 2, kDecimMaxFactor = 16, kDecimMaxTaps = 512, kDecimMaxShift = 16;
constexpr uint32_t kDecimHistWords = 512;   // a history buffer: the last n_taps - 1 inputs, widened, at [0, n_taps - 1)
struct DecimParams {
    const void *src;            // the call's inputs in `format`, 16-byte aligned
    uint64_t n_in;              // ... how many (> 0)
    const uint32_t *hist_prev;  // the n_taps - 1 inputs in front of the call (zero where the stream had not begun)
    uint32_t *hist_next;        // ... and in front of the next one (the other buffer)
    const int32_t *taps;        // device memory, padded with zeros to a multiple of eight
    const uint16_t *u8_table;   // 8-bit input: the widening table (device memory), else null
    uint32_t *out;              // CS16 dwords
    uint64_t n_out;             // outputs of the call (may be 0: only the history moves on)
    uint32_t factor, n_taps, shift;
    uint32_t first;             // input index of the call's first output: (-P) mod factor
    uint32_t row_len;           // decim_row_len(factor, n_taps): dwords per polyphase row in LDS
    uint32_t recip;             // ceil(2^20 / factor)
    MixParams mix;              // the mixer (period 0: none)
    // after everything else, so that the CS16 and 8-bit instantiations see the layout they always had
    uint32_t format;            // InFormat (kIn8Bit exactly when u8_table is set)
    float scale;                // CF32: g of q(x) = clamp(rint(x g)); means nothing to the other formats
};
uint32_t decim_row_len(uint32_t factor, uint32_t n_taps);
int launch_decim(const DecimParams &p, void *stream);
// Resampling (adsb_resamp_*; adsb_resamp.hip: k_resamp, k_resamp_history): one call's inputs -> its outputs at up / down
// times the rate and the history the next call starts from.  A kernel of its own beside the decimator's.
constexpr uint32_t kResampMaxRatio = 128, kResampMaxTaps = 4096, kResampMaxPhaseTaps = 512, kResampMaxShift = 16;
constexpr uint32_t kResampHistWords = 512;     // a history buffer: the last K - 1 inputs, widened, at [0, K - 1)
constexpr uint32_t kResampLdsWords = 16384;    // 64 KB per workgroup at most
struct ResampParams {
    const void *src;            // the call's inputs in `format`, 16-byte aligned
    uint64_t n_in;              // ... how many (> 0)
    const uint32_t *hist_prev;  // the K - 1 inputs in front of the call (zero where the stream had not begun)
    uint32_t *hist_next;        // ... and in front of the next one (the other buffer)
    const int32_t *taps;        // device memory in polyphase order: [phase p][j] = h[p + j up], k_pad to a phase, zero-padded
    const uint16_t *u8_table;   // 8-bit input: the widening table (device memory), else null
    uint32_t *out;              // CS16 dwords (4-byte aligned; 16-byte aligned: 16-byte stores)
    uint64_t n_out;             // outputs of the call (may be 0: only the history moves on)
    uint32_t up, down;          // L, M
    uint32_t k_taps, k_pad;     // K = ceil(T / L), and K rounded up to a multiple of eight
    uint32_t shift;
    uint32_t p0, q0;            // the call's first output n0: (n0 M) mod L, and floor(n0 M / L) - P (its newest input, in the call)
    uint32_t rows;              // R = resamp_rows(up, down): a workgroup takes up x R outputs
    uint32_t row_len;           // resamp_row_len(down, rows, k_taps): dwords per polyphase row in LDS
    uint32_t recip_up, recip_down;   // ceil(2^32 / L), ceil(2^32 / M) (unused where the divisor is 1)
    MixParams mix;              // the mixer (period 0: none)
    // after everything else, so that the CS16 and 8-bit instantiations see the layout they always had
    uint32_t format;            // InFormat (kIn8Bit exactly when u8_table is set)
    float scale;                // CF32: g of q(x) = clamp(rint(x g)); means nothing to the other formats
};
uint32_t resamp_rows(uint32_t up, uint32_t down);
uint32_t resamp_row_len(uint32_t down, uint32_t rows, uint32_t k_taps);
uint32_t resamp_lds_words(uint32_t up, uint32_t down, uint32_t rows, uint32_t k_taps);
int launch_resamp(const ResampParams &p, void *stream);
// Resampler banks (adsb_bank_*; adsb_resamp.hip: k_resamp_bank, k_resamp_bank_history): many calls of one ratio and one
// filter in one launch.  What a call has of its own -- a ResampParams' src, n_in, out, n_out, hist_prev, hist_next, p0,
// q0 and mix.phase -- comes from descriptor blockIdx.y in device memory; everything else stays in the launch's parameters.
constexpr uint32_t kResampBankMaxRuns = 16384;   // ADSB_MAX_RECEIVERS (the grid's y extent: 65535 at most)
struct ResampBankRun {
    const void *src;
    uint64_t n_in;              // (> 0: a run without input is not described)
    uint32_t *out;
    uint64_t n_out;
    const uint32_t *hist_prev;
    uint32_t *hist_next;
    uint32_t p0, q0;
    uint32_t mix_phase;         // P mod N of this run's stream (0 without a mixer)
    uint32_t reserved;
};
// `common`: a ResampParams whose per-call fields mean nothing; `runs`: the descriptors as the host sees them (checked here,
// each as launch_resamp checks a call), `d_runs`: the same in device memory, complete before the launch on `stream`.  The
// grid is (tiles of the longest run) x n_runs: a workgroup past its run's last output returns at once.
int launch_resamp_bank(const ResampParams &common, const ResampBankRun *runs, const ResampBankRun *d_runs, uint32_t n_runs,
                       void *stream);
// Input statistics (adsb_instat_*; adsb_instat.hip: k_instat, k_instat_bank): the raw input of a decimator's, resampler's
// or bank's call counted into adsb_input_stats records in device memory.  A kernel of its own in front of the filter's,
// with parameters of its own.  A tile is what a workgroup reads in one round: kInstatThreads x kInstatUnroll 16-byte
// loads; a launch has kInstatMaxGroups workgroups per run at most, each taking every gridDim.x-th tile.
constexpr int kInstatThreads = 256, kInstatUnroll = 4;
constexpr uint32_t kInstatMaxGroups = 1024;
constexpr uint32_t kInstatBankGroups = 4096;   // a bank's launch: about this many workgroups over all its runs
__host__ __device__ constexpr uint32_t instat_tile_samples(uint32_t format)
{
    return (uint32_t)(kInstatThreads * kInstatUnroll) * (16u / in_bytes_per_sample(format));
}
struct InstatParams {
    const void *src;            // the call's inputs in `format`, 16-byte aligned (a bank: from the descriptors)
    uint64_t n_in;              // ... how many (> 0)
    const uint16_t *u8_table;   // 8-bit input: the widening table (device memory), else null
    unsigned long long *acc;    // device memory: n_streams records, each laid out as adsb_input_stats
    uint32_t n_streams;         // 1; a bank: its N (a descriptor's `reserved` is the stream, below N)
    uint32_t format;            // InFormat
    float scale;                // CF32: g
};
int launch_instat(const InstatParams &p, void *stream);
// `runs` / `d_runs`: the descriptors of launch_resamp_bank, on the host (checked here) and in device memory
int launch_instat_bank(const InstatParams &common, const ResampBankRun *runs, const ResampBankRun *d_runs, uint32_t n_runs,
                       void *stream);
// Receiver seams (adsb_set_receiver_carry; adsb_seam.hip): the first kLead positions of every buffer of a receivers pass
// tried against a lead-in that holds the end of the same receiver's previous buffer.  Kernels of their own beside the
// scan, with parameters of their own -- ScanParams and the scan's instantiations stay as they are.
constexpr uint32_t kSeamWorstPerChunk = 5u * (uint32_t)kLead;   // every seam position sliced, five trials each
struct SeamDesc {            // per buffer of a pass, written by the host into mapped memory (host::seam_prev_map)
    int32_t prev;            // the previous buffer of this buffer's receiver in the same pass, or -1: the receiver's carry
    uint32_t rx;             // the buffer's receiver
    uint32_t last;           // 1: no later buffer of the pass belongs to that receiver (its end becomes the carry)
    uint32_t reserved;
};
struct SeamCounters {        // device memory, all zero between passes (k_seam_match leaves them so)
    uint32_t n_list, n_rec, overflow, reserved;   // overflow: bit 0 the record block, bit 1 the seam list
    unsigned long long rec_sum;                   // 64-bit sum of every u64 word of the records written
};
struct SeamSummary {         // mapped host memory, eight separate posted writes, `seq` issued last
    uint32_t n_rec, overflow, rec_sum_lo, rec_sum_hi, n_list, reserved;
    uint32_t check;          // seam_summary_check() of the six words above and seq
    uint32_t seq;
};
__host__ __device__ inline uint32_t seam_summary_check(const uint32_t w[6], uint32_t seq)
{
    uint32_t x = 0x5EA3C0DEu ^ (seq * 2654435761u);
    for (int k = 0; k < 6; k++) x ^= (w[k] << (k + 3)) | (w[k] >> (29 - k));
    return x;
}
struct SeamParams {
    const void *src;         // the pass's IQ: CS16 dwords or CU8 byte pairs
    uint64_t n_samples;
    uint32_t n_chunks;       // buffers of the pass
    uint32_t first_chunk;    // k_seam_scan: the launch takes buffers [first_chunk, first_chunk + n_scan)
    uint32_t n_scan;
    const uint16_t *u8_table;   // CU8: the widening table (device memory), else null
    const SeamDesc *desc;    // n_chunks, mapped host memory
    uint32_t *carry;         // n_receivers rows of kCarrySamples CS16 dwords
    uint32_t n_receivers;
    uint32_t *lead;          // n_chunks rows of kCarrySamples CS16 dwords: the samples in front of each buffer
    uint32_t *bitmap;        // the pass's address superset (ScanParams::bitmap)
    uint32_t bitmap_lg;
    const uint32_t *tables;  // ScanParams::tables
    uint32_t fix;            // ScanParams::fix
    uint32_t emit_all;       // the redo after an overflow: address/parity trials are records too (no list, no match);
                             // what it learns goes into `bitmap` all the same -- the bitmap in use at the redo, which an
                             // icao_flush behind the pass may have made another one than the first run's
    TrialRecord *list;       // address/parity trials with their sliced bytes and power, device memory
    uint32_t list_cap;
    TrialRecord *rec;        // finished records, mapped host memory
    uint32_t rec_cap;
    SeamCounters *ctr;
    SeamSummary *summary;    // mapped host memory
    uint32_t seq;
    // receiver seams scored on the device (adsb_set_receiver_carry_scoring), both null everywhere else -- the kernels then
    // do what they always did: a mirror of `rec` in device memory (rec_cap entries: the device-side merge never reads
    // records back out of mapped host memory), and the word pair where k_seam_match leaves (n_rec, overflow) before it
    // zeroes the counters.  After everything else, so that the fields above stay where they were.
    TrialRecord *rec_dev;
    uint32_t *note;
};
int launch_seam_lead(const SeamParams &q, void *stream);    // k_rx_lead, then k_rx_carry_update
int launch_seam_scan(const SeamParams &q, void *stream);    // k_seam_scan
int launch_seam_match(const SeamParams &q, void *stream);   // k_seam_match: the list against the bitmap, then the summary
// Receiver seams scored on the device (adsb_seam_score.hip; adsb_seam_score_dev.h has the index arithmetic): in front of
// k_rx_adders on the score stream, the pass's seam records are merged into the records kernel's ordered arrays and the
// pass's own hits at j < kLead dropped -- into a second set of arrays, which the three keyed kernels then take for the
// pass's.  The first set stays as the records kernel left it (the host fetches ScoreDev::rec when it refuses the result).
struct SeamMergeState {      // device memory, per slot; ticket and bad are zero between passes
    uint32_t n_own;          // ScoreState::n as the records kernel left it
    uint32_t n_seam;         // seam records of the pass (the note's n_rec)
    uint32_t go;             // 1: the merged arrays are to be written and ScoreState::n is the merged count
    uint32_t ticket;         // k_seam_place: workgroups that have finished (the last one cleans up)
    uint32_t bad;            // k_seam_mark: a record that cannot be placed (a buffer or key out of range, a key twice)
    uint32_t reserved[3];
};
struct SeamMergeSummary {    // mapped host memory, `seq` issued last
    uint32_t merged;         // 1: the pass came scored from the records kernel and went through the merge
    uint32_t n_seam;         // seam records merged
    uint32_t dropped;        // own hits dropped for j < kLead
    uint32_t unscored;       // 1: the merge declared the pass unscored (seam overflow, more merged hits than ScoreDev::cap)
    uint32_t reserved[3];
    uint32_t seq;
};
struct SeamMergeParams {
    const TrialRecord *seam_rec;   // SeamParams::rec_dev
    uint32_t seam_cap;             // ... and its entries
    uint32_t *note;                // SeamParams::note; the merge zeroes it
    ScoreDev merged;               // the pass's ScoreDev with rec, si, pos, slot and flag pointing at the merged arrays
    uint32_t *present;             // n_chunks rows of kSeamKeyStride words: bit 5 j + try_phase - 4 of row b, all zero between passes
    uint32_t *own_start;           // n_chunks + 1: the first own hit of every buffer
    uint32_t *drop;                // n_chunks: own hits with j < kLead, all zero between passes
    uint32_t *seam_base;           // n_chunks: where the buffer's first seam record lands
    uint32_t *own_shift;           // n_chunks: what a kept own hit's index moves by
    SeamMergeState *st;
    SeamMergeSummary *summary;
    uint32_t seq;
};
// k_seam_mark, k_seam_prefix, k_seam_place on `stream`, in that order; p: the pass's own parameters (p.score: the records
// kernel's arrays, the plain first-adder table -- emptied here -- and the state)
int launch_seam_merge(const ScanParams &p, const SeamMergeParams &m, void *stream);
// self-test: out[i] = the repair k_score finds for residuals[i] under `mode` (adsb_fix_dev.h: fix_lookup), device memory
int launch_fix_lookup(const uint32_t *tables, const uint32_t *d_residuals, uint32_t n, uint32_t mode, uint32_t *d_out, void *stream);

}  // namespace adsb
