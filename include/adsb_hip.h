/*
 * include/adsb_hip.h -- C ABI of libadsb_hip.so, the MI355X (gfx950) drop-in for the
 * demod_2400 hot path of rsadsb/dump1090_rs v0.8.1.
 *
 * The reference has no FFI or plugin interface of its own: the boundary it offers
 * is its Rust library API.  Each entry point below replaces one of those items; a
 * Rust host declares them in an `extern "C"` block and keeps its own
 * to_mag / demodulate2400 / ModeSMessage wrappers (INTEGRATION.md shows the stub).
 *
 *   reference item (file:line)                              replaced by
 *   ------------------------------------------------------  -------------------------
 *   utils::to_mag                  src/utils.rs:43-58       adsb_to_mag
 *   MagnitudeBuffer / push         src/lib.rs:30-51         the (data[131398], length) pair
 *   demod_2400::demodulate2400     src/demod_2400.rs:115    adsb_demodulate2400
 *   ModeSMessage / buffer()        src/demod_2400.rs:92-112 adsb_msg (msg, len)
 *   icao_filter::icao_flush        src/icao_filter.rs:11    adsb_icao_flush
 *   to_mag + demodulate2400 per buffer, as composed at
 *     dump1090_rs/src/main.rs:166-167 and
 *     benches/demod_benchmark.rs:10-11                      adsb_demod_iq / _device
 *
 * Conventions: every function returns ADSB_OK (0) or a negative adsb_status and
 * never throws, aborts or panics across the ABI (an allocation that fails inside
 * comes back as ADSB_ERR_NOMEM); the caller owns every host
 * buffer; all pointers are plain host pointers except where the name says
 * `device`.  After ADSB_ERR_HIP or ADSB_ERR_NOMEM from a demodulating call the
 * pass it was working on is lost and the filter may have seen part of it: an
 * adsb_ctx is then best destroyed and made anew (or adsb_icao_flush'ed, if starting
 * from an empty filter is acceptable); an adsb_multi says so itself
 * (ADSB_ERR_POISONED) and restarts on adsb_multi_icao_flush.  One adsb_ctx per host thread / per GPU: the ICAO address filter
 * (process-global statics in the reference, src/icao_filter.rs:8-9) lives in the
 * context, so contexts are independent streams (one context can also serve many receivers, each with a filter of
 * its own: "Many receivers, one pass").  There is no CPU fallback:
 * adsb_create fails with ADSB_ERR_NO_DEVICE when no gfx950 device is usable.
 * The host side of the library is built for x86-64 Linux hosts (its spin loops are
 * the `pause` instruction; thread placement reads sysfs): the hosts MI355X boards sit in.
 */
#ifndef ADSB_HIP_H
#define ADSB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* src/lib.rs:22-26 */
#define ADSB_MODES_MAG_BUF_SAMPLES 131072u
#define ADSB_TRAILING_SAMPLES 326u
#define ADSB_MODES_LONG_MSG_BYTES 14u
#define ADSB_MODES_SHORT_MSG_BYTES 7u
/* length of MagnitudeBuffer.data, src/lib.rs:31 */
#define ADSB_MAG_DATA_LEN (ADSB_TRAILING_SAMPLES + ADSB_MODES_MAG_BUF_SAMPLES)

typedef enum {
    ADSB_OK = 0,
    ADSB_ERR_INVALID = -1,   /* null pointer / bad argument */
    ADSB_ERR_NO_DEVICE = -2, /* no usable HIP device (there is no CPU fallback) */
    ADSB_ERR_HIP = -3,       /* a HIP runtime call failed; see adsb_last_error */
    ADSB_ERR_TOO_LONG = -4,  /* more than 131072 samples handed to a one-buffer call:
                                the reference panics here (src/lib.rs:48) */
    ADSB_ERR_CAPACITY = -5,  /* `out` too small; *n_out holds the required count and the
                                first `cap` messages were written.  The pass itself is done (the
                                filter has advanced, as after demodulate2400 returned its Vec):
                                do not repeat the call -- adsb_fetch_messages hands out the whole
                                list, which the context keeps until its next demod call */
    ADSB_ERR_NOMEM = -6,
    ADSB_ERR_BUSY = -7,      /* submissions pending where none are allowed, or too many in flight */
    ADSB_ERR_POISONED = -8   /* an adsb_multi one of whose captures failed: what it computed after that capture is
                                not the single stream's any more, so nothing further is accepted or returned until
                                adsb_multi_icao_flush (with nothing in flight) has started the stream over */
} adsb_status;

#define ADSB_MAX_IN_FLIGHT 4
/* ... and for a context created with max_chunks <= 16, whose passes are a single launch each
 * (adsb_max_in_flight tells which a context got) */
#define ADSB_MAX_IN_FLIGHT_SMALL 8

typedef struct adsb_ctx adsb_ctx;

/* Mirrors ModeSMessage (src/demod_2400.rs:92-102) plus provenance.
 * buffer() == msg[0..len]. */
typedef struct {
    uint8_t msg[ADSB_MODES_LONG_MSG_BYTES];
    uint8_t len;       /* 7 (MsgLen::Short) or 14 (MsgLen::Long) */
    uint8_t try_phase; /* winning trial phase, 4..8 (demod_2400.rs:158) */
    int32_t score;     /* src/mode_s/mod.rs score of the winning trial */
    uint32_t j;        /* preamble index into MagnitudeBuffer.data */
    uint64_t chunk;    /* index of the 131072-sample buffer inside this call */
    double signal_level;
} adsb_msg;

/* Counters of the most recent demod call (diagnostics / bench). */
typedef struct {
    uint64_t n_samples;
    uint64_t n_chunks;
    uint64_t n_candidates;  /* j that passed preamble + SNR + quiet gates */
    uint64_t n_ap_entries;  /* address/parity trials deferred to the filter match */
    uint64_t n_records;     /* trial records replayed on the host */
    uint64_t n_messages;
    float ms_scan;          /* scan kernel (IQ -> candidates -> trials), HIP events */
    float ms_match;         /* address/parity match kernel */
    float ms_records;       /* record builder kernel */
    float ms_total_device;  /* first launch -> last kernel end */
    uint32_t retries;       /* device-list overflow fallbacks taken */
    float ms_scan_exclusive; /* the part of ms_scan after the previous pass's scan had finished: consecutive
                              * pipelined scans overlap (the next one's workgroups fill the CUs as the previous
                              * grid drains), so the sum of ms_scan over passes counts the overlap twice while
                              * the sum of ms_scan_exclusive is the device time the scans took altogether */
} adsb_stats;

/* Create a context on HIP device `device` (>= 0), sized to demodulate up to
 * `max_chunks` 131072-sample buffers per call (host-pointer calls stage through
 * a device buffer of that size; device-pointer calls only size the lists).
 * A context created with max_chunks <= 16 is one for the reference's own call shape (one read, one
 * demodulation, dump1090_rs/src/main.rs:161-167): each of its passes is a single kernel launch, and it
 * keeps ADSB_MAX_IN_FLIGHT_SMALL (8) of them in flight instead of ADSB_MAX_IN_FLIGHT (4).
 * Footprint (each pass in flight has its own lists):
 *   device   the address supersets the match tests against, one more than passes in flight in rotation: 2 MiB each
 *            (bit a = address a) in a large context, plus two for the device-side copy of the filter; 64 KB each
 *            (2^19 bits, address folded: a superset is all the match needs) in a context created with
 *            max_chunks <= 16, which never scores on the device.  Per pass in flight the address/parity list, the
 *            hit list with the scan's bit fields per hit, and (large contexts) the scoring buffers: ~0.8 MB each for
 *            max_chunks = 1 (~7 MB in all, 0.6 of them bitmaps), ~109 MB each for 512 (~450 MB in all);
 *   pinned host (mapped, written by the kernels; one allocation per context)  per pass in flight 32 B per trial
 *            record (4096 + 1024 max_chunks of them) + in large contexts 44 B per scored message slot
 *            (min(that, 262144)): ~1.3 MB in all for max_chunks = 1, ~115 MB for 512; host-pointer calls of a few
 *            buffers add a pinned staging buffer of their size, the ring its slots.
 * Input denser than the lists are sized for (several times a busy airspace) is still
 * demodulated exactly, buffer by buffer through worst-case lists allocated on first use
 * (another 10 MB of device and 20 MB of pinned memory; stats.retries).
 * adsb_set_receivers(n) adds 16 KB of ordinary host memory per receiver beyond the first, adsb_set_receiver_scoring what
 * its paragraph lists ("Many receivers, one pass"). */
int adsb_create(adsb_ctx **out, int device, size_t max_chunks);
void adsb_destroy(adsb_ctx *ctx);

/* Order the context's work behind the caller's HIP stream (e.g. torch's current stream)
 * instead of the context's own: whatever that stream has been given before a call (the
 * kernels or copies that produce the IQ) is complete before the pass reads its input.  The
 * passes themselves run on the context's internal streams; their results are handed over
 * by the blocking call or by adsb_collect, not through the stream.  Pass NULL to go back to
 * the private stream. */
int adsb_set_stream(adsb_ctx *ctx, void *hip_stream);
/* HIP-event timing of the kernels: 0 = off, 1 = ms_scan only (default; two events),
 * 2 = also ms_match / ms_records / ms_total_device (an event costs the
 * stream several microseconds, so level 2 slows a call down noticeably).
 * Values below 0 count as 0, values above 2 as 2.
 * The level never changes a result: every entry point returns the same messages, signal records and
 * filter tables at every level (tests/test_gpu_profiling_levels.py holds levels 0 and 2 to the CPU
 * oracle).  It does change which code a pass runs through.  At level 2 the kernels are kept apart to be
 * timed: no pass is a single launch (a context created with max_chunks <= 16 runs scan, match and records
 * as three launches on one of two scan streams instead of one launch on one of four), a ring slot is never
 * read in place (it is copied in front of its pass), and adsb_host_rematches does not grow (no pass is
 * launched unordered and matched again by the host: the stream order does it).  At level 0 the passes are
 * those of level 1 without their events, and every ms_* field of adsb_stats is 0.
 * Returns ADSB_ERR_BUSY while passes are pending (submitted and not yet collected) or a shard is parked
 * between adsb_shard_scan and adsb_shard_finish; the level then stays what it was. */
int adsb_set_profiling(adsb_ctx *ctx, int level);

/* == icao_filter::icao_flush() (src/icao_filter.rs:11-17) for this context.  Stream-ordered: costs nothing by
 * itself; the next pass starts on the next address superset of the rotation (a large context's is clean already,
 * a context for passes of a few buffers has that pass clear its 64 KB when it starts) and waits for no pass in
 * flight -- a flush before every pipelined call, the reference's benchmark shape (benches/demod_benchmark.rs:9),
 * costs the same as none. */
int adsb_icao_flush(adsb_ctx *ctx);

/* == utils::to_mag (src/utils.rs:43-58).  iq_re_im is the in-memory
 * Complex<i16> order: first i16 = re, second = im.  data_out must hold
 * ADSB_MAG_DATA_LEN u16: [0,326) zero, [326,326+n) magnitudes, rest zero.
 * n > 131072 -> ADSB_ERR_TOO_LONG. */
int adsb_to_mag(adsb_ctx *ctx, const int16_t *iq_re_im, size_t n, uint16_t *data_out,
                size_t *length_out);

/* == demod_2400::demodulate2400 (src/demod_2400.rs:115-212) on one
 * MagnitudeBuffer given as (data[ADSB_MAG_DATA_LEN], length).  Messages come
 * out in ascending j, exactly the reference's Vec order. */
int adsb_demodulate2400(adsb_ctx *ctx, const uint16_t *data, size_t length, adsb_msg *out,
                        size_t cap, size_t *n_out);

/* to_mag + demodulate2400 over consecutive 131072-sample buffers of a host IQ
 * stream of any length (the last buffer may be short), the filter persisting
 * from buffer to buffer as in dump1090_rs/src/main.rs:154-167.  Output order:
 * ascending (chunk, j). */
int adsb_demod_iq(adsb_ctx *ctx, const int16_t *iq_re_im, size_t n_samples, adsb_msg *out,
                  size_t cap, size_t *n_out);

/* Same, the IQ already resident in device memory (16-byte aligned). */
int adsb_demod_iq_device(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples,
                         adsb_msg *out, size_t cap, size_t *n_out);

/* Asynchronous form of adsb_demod_iq_device for a host that keeps the GPU fed: enqueue one
 * pass (kernels + result copy) and return at once; at most ADSB_MAX_IN_FLIGHT passes
 * (adsb_max_in_flight) may be pending.  adsb_collect waits for the OLDEST pending pass, replays it through the
 * filter and returns its messages, so results come back in submission order and the
 * host replay of pass i overlaps the device scan of pass i+1.  adsb_icao_flush applies
 * to the passes submitted after it.  The synchronous calls return ADSB_ERR_BUSY while
 * anything is pending.  device_iq must stay valid and unchanged until its collect.  One
 * submission holds at most the max_chunks buffers the context was created for
 * (ADSB_ERR_INVALID beyond that; adsb_demod_iq_device cuts longer inputs into such passes
 * itself). */
int adsb_submit_iq_device(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples);
int adsb_collect(adsb_ctx *ctx, adsb_msg *out, size_t cap, size_t *n_out);
int adsb_pending(const adsb_ctx *ctx);
/* How many passes this context lets be in flight: ADSB_MAX_IN_FLIGHT, or ADSB_MAX_IN_FLIGHT_SMALL for a
 * context created for at most 16 buffers per pass (the ring of such a context has that many slots). */
int adsb_max_in_flight(const adsb_ctx *ctx);

/* The complete message list of the most recent call that returned ADSB_ERR_CAPACITY
 * (adsb_demodulate2400, adsb_demod_iq[_device], adsb_collect): that call already ran the pass and
 * updated the filter, so repeating it would score against a different filter; this returns what it
 * produced.  The list is kept until the next of those calls.  ADSB_ERR_INVALID when nothing is held. */
int adsb_fetch_messages(adsb_ctx *ctx, adsb_msg *out, size_t cap, size_t *n_out);

/* Streaming ring for a host that produces IQ (an SDR read loop, dump1090_rs/src/main.rs:
 * 154-167): adsb_max_in_flight() (4 or 8) pinned host buffers of `samples_per_slot` samples (4 bytes
 * each) with a device staging buffer each.  Fill the buffer adsb_ring_acquire hands out (e.g.
 * read the SDR straight into it), adsb_ring_submit(n) starts the slot's pass -- one launch that
 * reads a slot of one or two buffers in place over the link; larger slots are copied first, on the
 * pass's own stream --, adsb_collect returns the oldest pass's messages.  While one slot's pass
 * runs, the next slots' transfers are in flight.  samples_per_slot may not exceed the
 * context's max_chunks buffers; adsb_ring_acquire returns ADSB_ERR_BUSY until the pass
 * that last used the slot has been collected. */
int adsb_ring_create(adsb_ctx *ctx, size_t samples_per_slot);
int adsb_ring_acquire(adsb_ctx *ctx, int16_t **host_iq_re_im, size_t *capacity_samples);
int adsb_ring_submit(adsb_ctx *ctx, size_t n_samples);
/* The same ring for CU8 input (see "8-bit IQ" below): slots of 2 * samples_per_slot bytes, filled with rtl_sdr's
 * bytes as they come; adsb_ring_submit and adsb_collect are shared.  A context has one ring, of one format:
 * adsb_ring_acquire on a CU8 ring, or adsb_ring_acquire_u8 on a CS16 ring, returns ADSB_ERR_INVALID. */
int adsb_ring_create_u8(adsb_ctx *ctx, size_t samples_per_slot);
int adsb_ring_acquire_u8(adsb_ctx *ctx, uint8_t **host_iq_re_im, size_t *capacity_samples);

/* ---------------------------------------------------------------------------------------------------------
 * 8-bit IQ (CU8), as an RTL-SDR delivers it: 2 bytes per sample, unsigned, I then Q -- byte 2k is `re` and byte
 * 2k + 1 `im` of sample k (the in-memory order of the CS16 calls above; read_test_data's [im][re] file order does
 * not apply).  A context widens every byte b through its table T (int16_t[256]): CU8 input b of n samples MEANS the
 * CS16 buffer widen(b), widen(b)[m] = T[b[m]] for every element m, and every _u8 call returns exactly what its CS16
 * twin returns on widen(b) -- the same adsb_msg fields in the same order, the same filter evolution, the same
 * carry-over behaviour (the carry is kept as widened CS16, so a stream may alternate the two formats) and the same
 * status codes.  The widening happens on the device, inside the kernels that read the samples; the zero lead-in,
 * the zero tail and the ragged end of a short buffer stay magnitude 0 (T[0] is a sample like any other).
 *
 * A new context's table is T_soapy, the one SoapyRTLSDR widens with (so that CU8 demodulates as the reference's
 * CS16 from that driver does): T_soapy[x] = (int16_t)(((float)x - 127.4f) * (1.0f / 128.0f) * 32767.0f), each
 * operation in f32, the conversion truncating.
 *
 *   adsb_set_u8_table         the context's table from now on (NULL: T_soapy again); applies to the passes submitted
 *                             after the call; ADSB_ERR_BUSY while passes are pending
 *   adsb_to_mag_u8, adsb_demod_iq_u8, adsb_demod_iq_device_u8, adsb_submit_iq_device_u8
 *                             the CS16 calls' arguments with CU8 IQ (device input 16-byte aligned); adsb_collect and
 *                             adsb_fetch_messages are shared */
int adsb_set_u8_table(adsb_ctx *ctx, const int16_t *table256);
int adsb_to_mag_u8(adsb_ctx *ctx, const uint8_t *iq_re_im, size_t n, uint16_t *data_out, size_t *length_out);
int adsb_demod_iq_u8(adsb_ctx *ctx, const uint8_t *iq_re_im, size_t n_samples, adsb_msg *out, size_t cap,
                     size_t *n_out);
int adsb_demod_iq_device_u8(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples, adsb_msg *out,
                            size_t cap, size_t *n_out);
int adsb_submit_iq_device_u8(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples);
/* The table a context widens with (ctx NULL: T_soapy as the library computes it, no device needed).  For the tests.
 * ADSB_ERR_BUSY while passes are pending. */
int adsb_selftest_u8_table(adsb_ctx *ctx, int16_t *out256);

/* For a host that keeps its own sample buffer (the Vec the SDR reads land in, dump1090_rs/src/main.rs:
 * 154-167, is allocated once): pin it and map it for the device, so that adsb_demod_iq on samples
 * INSIDE it (16-byte aligned start, at most 16 buffers) reads them in place over the link -- one kernel
 * launch, no copy of the samples on the host.  The memory stays the caller's; it must not be freed
 * before adsb_host_unregister (adsb_destroy unregisters what is left).  Samples outside any registered
 * range take the usual path.  ADSB_ERR_INVALID for a range that overlaps a registered one. */
int adsb_host_register(adsb_ctx *ctx, void *host_ptr, size_t bytes);
int adsb_host_unregister(adsb_ctx *ctx, void *host_ptr);

/* src/utils.rs:23-40 read_test_data: file pairs are [im][re] little-endian;
 * writes in-memory {re, im}.  Returns samples read via *n_out. */
int adsb_read_test_data(const char *path, int16_t *iq_re_im, size_t max_samples, size_t *n_out);

/* The raw output line of dump1090_rs/src/main.rs:172-176 for one message:
 * "*" + lowercase hex of buffer() + ";\n" (the format port 30002 clients such as adsb_deku's
 * radar read).  Writes 17 or 31 characters plus a terminating NUL into out (>= 32 bytes);
 * returns the length without the NUL, or a negative status.  Host only. */
int adsb_format_raw(const adsb_msg *msg, char *out, size_t out_size);

/* One trial message as the device hands it to the host replay. */
typedef struct {
    uint64_t power;   /* bits 0..39: sum of the 33 squared magnitudes from j+19 (demod_2400.rs:
                       * 191-196; below 2^38); bits 40..63: see pad */
    uint32_t chunk;
    uint32_t j_tp;    /* j | try_phase << 24 */
    uint8_t msg[ADSB_MODES_LONG_MSG_BYTES];
    uint16_t pad;     /* 0: nothing more.  Records from adsb_shard_finish set bit 0: bits 40..63 of
                       * `power` hold the CRC residual of msg over its own length (src/crc.rs:263-282),
                       * which spares adsb_replay_records the walk over the bytes; and bit 1: bits 4..15
                       * hold icao_hash (src/icao_filter.rs:19-43) of the value the message's DF asks the
                       * filter about -- the residual for DF 0,4,5,16,20,21,24-31, else the address.  For a
                       * DF17/18 with a non-zero residual (one that ADSB_FIX_1BIT may repair) that hash is the
                       * damaged address's: the replay does not use it, it hashes the repaired address itself. */
} adsb_trial;

/* Carry-over mode -- opt-in and NOT the reference's semantics.  dump1090_rs starts every
 * MagnitudeBuffer with 326 zero samples (src/lib.rs:24,36-44; the constant is what upstream
 * C dump1090 uses to carry the end of the previous buffer over), so a frame that straddles
 * two buffers is lost.  With carry-over enabled the lead-in of every 131072-sample buffer
 * holds the 326 samples that preceded it in the stream -- within a call and from the
 * previous call on this context -- and such frames are decoded in the later buffer
 * (j < 326 there).  Applies to the IQ entry points (adsb_demod_iq*, submit/collect, the
 * ring); adsb_to_mag / adsb_demodulate2400 keep working on the caller's buffer as is.
 * Enabling or disabling restarts the stream (nothing precedes the next call).  Returns
 * ADSB_ERR_BUSY while passes are pending. */
int adsb_set_carry_over(adsb_ctx *ctx, int enabled);

/* Error correction -- opt-in, off by default; with ADSB_FIX_NONE every output is the reference's.
 * ADSB_FIX_1BIT repairs extended squitters with one flipped bit, as upstream C dump1090 does, and changes one branch
 * of score_modes_message (src/mode_s/mod.rs:91-109) and nothing else:
 *   a DF 17 / 18 trial (112 bits) whose residual c = modes_checksum(msg, 112) is non-zero is looked up among the
 *   syndromes syn(b) = modes_checksum(e_b, 112) of the single-bit messages e_b (bit 0 = MSB of byte 0), b = 5..111
 *   (bits 0..4 are the DF: repairing them would change the message's class and length).  The 107 syndromes are
 *   distinct and non-zero, so c names at most one b.  When c == syn(b), m' = msg ^ e_b and addr' = bits 9..32 of m'
 *   (a flip in bits 8..31 changes the address); the trial scores ADSB_SCORE_FIXED_1BIT if icao_filter_test(addr')
 *   (DF18 too, with the plain address), else -1, and adds nothing to the filter.  Any other c still scores -2.
 * Selection is unchanged (best of the five phases by strict >, from -2; emitted when >= 0).  1200 sits below a clean
 * DF17 (1800 / 1400) and a known DF11 IID 0 (1600), above address/parity (1000) and a new DF11 (750), and occurs nowhere
 * in the reference: score == ADSB_SCORE_FIXED_1BIT marks a repaired message, whose msg holds the corrected bytes m'
 * (signal_level, j, try_phase and chunk as for any message).  DF11 is not repaired: its IID is folded into the low
 * 7 bits of the residual, where a flipped bit cannot be told from an IID.
 * The mode applies to every demod entry point of the context (blocking, submit/collect, the ring, the _u8 twins,
 * adsb_demodulate2400, carry-over, adsb_shard_scan / finish) for the passes submitted after the call.  Other values:
 * ADSB_ERR_INVALID; ADSB_ERR_BUSY while passes are pending.  adsb_get_error_correction returns the mode in effect
 * (ADSB_ERR_INVALID for a null context). */
#define ADSB_FIX_NONE 0
#define ADSB_FIX_1BIT 1
#define ADSB_SCORE_FIXED_1BIT 1200
/* ADSB_FIX_2BIT repairs one OR two flipped bits (1 | 2: a superset of ADSB_FIX_1BIT; the value 2 is ADSB_ERR_INVALID
 * everywhere), as upstream C dump1090's --aggressive does.  It changes the same branch, DF 17 / 18 with c != 0:
 *   if c == syn(b) for b in 5..111, the trial is scored exactly as under ADSB_FIX_1BIT (1200 or -1);
 *   else if c == syn(a) ^ syn(b) for 5 <= a < b <= 111, m' = msg ^ e_a ^ e_b, addr' = bits 9..32 of m', and the trial
 *   scores ADSB_SCORE_FIXED_2BIT if icao_filter_test(addr') (DF18 too, with the plain address), else -1, and adds
 *   nothing to the filter; any other c still scores -2.
 * The 5671 pair syndromes are distinct, non-zero and none is a single bit's, so c names at most one repair.  1100 sits
 * below a single-bit repair (1200), above address/parity (1000), and occurs nowhere in the reference or mode 1; the
 * msg of a 1100 message holds the corrected bytes.  It reaches every entry point ADSB_FIX_1BIT does. */
#define ADSB_FIX_2BIT 3
#define ADSB_SCORE_FIXED_2BIT 1100
int adsb_set_error_correction(adsb_ctx *ctx, int mode);
int adsb_get_error_correction(const adsb_ctx *ctx);

/* ---------------------------------------------------------------------------------------------------------
 * Signal statistics -- opt-in, off by default; with the mode off nothing observable changes (the same frames, the
 * same kernels launched, the same footprint).  With it on every pass also delivers one small integer record per
 * 131072-sample buffer: what a receiver's gain is tuned by -- where the noise floor sits, how hot the loudest samples
 * are, how much of the stream hits the ADC rails.  The magnitudes never exist in memory on the IQ path, so they are
 * counted on the device, by a kernel of its own beside the scan that reads the pass's input once more.
 *
 * Buffer c of a call has n valid samples; its magnitudes are m[k] = to_mag(iq)[k], the u16 values adsb_to_mag returns
 * and the scan computes (the same device function; _u8 input is first widened through the context's table).  The
 * zero lead-in, the zero tail and the samples carried over from the previous buffer under adsb_set_carry_over are
 * NOT counted.  Every field is an exact integer: it equals the plain restatement, whatever order the device adds in. */
#define ADSB_SIGNAL_BINS 60
typedef struct adsb_signal_stats {
    uint64_t chunk;      /* index of the buffer inside the call, as adsb_msg.chunk */
    uint64_t sum_power;  /* sum of m[k]^2  (< 2^49) */
    uint32_t n_samples;  /* n */
    uint32_t peak;       /* max m[k], 0 for an empty buffer */
    uint32_t n_strong;   /* samples with 2*m^2 >= 65535^2  (above -3 dBFS) */
    uint32_t n_clipped;  /* samples with a component at a rail: CS16 re or im in {-32768, 32767};
                            CU8 a byte in {0, 255} (on the bytes, before widening) */
    uint32_t hist[60];   /* hist[adsb_signal_bin(m[k])]++  (ADSB_SIGNAL_BINS of them) */
} adsb_signal_stats;     /* 272 bytes */

/* What a gain display shows, over any number of records (adsb_signal_summary). */
typedef struct adsb_signal_summary_t {
    uint64_t n_buffers;
    uint64_t n_samples;
    double mean_power_dbfs;  /* 10 log10(sum of sum_power / n_samples / 65535^2) */
    double peak_dbfs;        /* 20 log10(max peak / 65535) */
    double median_dbfs;      /* the noise floor, which aircraft bursts do not move: 20 log10(e / 65535), e the lower edge
                                of the bin that holds the (n_samples + 1) / 2-th smallest magnitude */
    double clipped_fraction; /* sum of n_clipped / n_samples (0 when there are no samples) */
    double strong_fraction;  /* sum of n_strong / n_samples */
} adsb_signal_summary_t;

#if defined(__GNUC__)
#define ADSB_MUST_CHECK __attribute__((warn_unused_result))
#else
#define ADSB_MUST_CHECK
#endif

/* adsb_set_signal_stats: the mode of the passes submitted after the call (ADSB_ERR_BUSY while passes are pending).  It
 * applies to every IQ entry point of the context -- adsb_demod_iq, adsb_demod_iq_device, submit / collect with 4 or 8
 * passes in flight, the ring in both formats, and all the _u8 twins; adsb_to_mag and adsb_demodulate2400, the caller's
 * magnitudes, are left alone, and adsb_shard_* / adsb_multi_* do not deliver records (out of scope: after adsb_shard_scan
 * adsb_fetch_signal_stats has none).  A pass that takes
 * the buffer-by-buffer overflow fallback, or that is redone through the three launches (adsb_host_rematches), still
 * delivers its records, computed once.  The first enable reserves 272 B x max_chunks of mapped host memory and as
 * much device memory (plus 4 B x max_chunks) per pass in flight; a context that never enables the mode keeps the
 * footprint documented at adsb_create.  Known cost: a ring slot of one or two buffers, which its pass reads in place
 * over the link, is read over the link a second time.
 * adsb_get_signal_stats: 1 / 0, or ADSB_ERR_INVALID for a null context. */
int adsb_set_signal_stats(adsb_ctx *ctx, int enabled);
int adsb_get_signal_stats(const adsb_ctx *ctx);
/* The records of the pass most recently collected (adsb_collect), or of the blocking call most recently returned: one
 * per buffer, in buffer order.  Like adsb_fetch_messages: *n_out is the full count even when `cap` is smaller (then the
 * first `cap` are written and the status is ADSB_ERR_CAPACITY); *n_out is 0, status ADSB_OK, when that pass ran with the
 * mode off or held no samples. */
ADSB_MUST_CHECK int adsb_fetch_signal_stats(adsb_ctx *ctx, adsb_signal_stats *out, size_t cap, size_t *n_out);
/* Quarter-octave bins of about 1.5 dB: m itself for m < 8; otherwise, with e = floor(log2 m) in 3..15,
 * 8 + 4 (e - 3) + ((m >> (e - 2)) & 3), at most 59.  Host only. */
int adsb_signal_bin(uint16_t m);
/* Sums n records into *out.  A logarithm of zero comes back as -inf (an all-zero capture, no samples at all), never
 * NaN.  Host only.  ADSB_ERR_INVALID for a null `out`, or a null `s` with n > 0. */
ADSB_MUST_CHECK int adsb_signal_summary(const adsb_signal_stats *s, size_t n, adsb_signal_summary_t *out);
/* Diagnostic: how many k_signal_stats launches this context has made (a pass with the mode off makes none). */
uint64_t adsb_selftest_signal_launches(const adsb_ctx *ctx);

/* ---------------------------------------------------------------------------------------------------------
 * Many receivers, one pass -- opt-in, off by default; with the mode off nothing observable changes.
 * One receiver produces 2.4 Msample/s: one 131072-sample buffer every 54.6 ms.  A host that gathers the IQ of many
 * receivers (an aggregator fed by a few hundred SDRs, a batch job over many recordings) can fill a deep pass only with
 * the buffers of all of them, and each receiver has an ICAO filter of its own.  adsb_set_receivers(ctx, n) gives the
 * context n filters; the _rx calls below take, beside the IQ, a map that names the receiver of every buffer.
 *
 * The map.  receiver_of_buffer[b], b = 0 .. ceil(n_samples / 131072) - 1, is the receiver buffer b of the call belongs
 * to, each < n.  The buffers of one receiver are consecutive buffers of THAT receiver's stream in ascending b, within a
 * call and from call to call.  Only the last buffer of a call may be short.  The map is a plain host array, copied
 * during the call: the caller may free it as soon as the call returns, also after a submit.  A blocking call longer
 * than max_chunks buffers is cut into passes as always; the map is indexed by the buffer's index in the CALL.
 *
 * What comes back is what n independent plain contexts would return: feed receiver r's buffers, one adsb_demod_iq call
 * per buffer, to a context r of its own; relabel every message's `chunk` with b; merge in ascending (chunk, j).  That
 * merged list is the list the _rx call returns, field for field, signal_level bit for bit, and
 * adsb_receiver_filter_table(r) equals context r's table A (4096 u32, src/icao_filter.rs:8) slot for slot.
 * adsb_collect, adsb_fetch_messages, ADSB_ERR_CAPACITY, adsb_get_stats and adsb_fetch_signal_stats (one record per
 * buffer) are shared with the plain calls and unchanged.
 *
 * How: the device does not know whose buffer it scans.  Every buffer starts from a zero lead-in, and the only state
 * the device keeps across buffers is the address SUPERSET the address/parity trials are matched against -- with
 * receivers on, the union of all receivers' addresses, which is a superset of each receiver's filter at every moment.
 * A false superset hit costs one trial record that the host replay then scores -1; what differs is that replay, which
 * scores every record against the filter of its buffer's receiver.  Unless adsb_set_receiver_scoring (below) says
 * otherwise, passes are never scored on the device while receivers are on (adsb_host_replays counts every pass); a pass
 * of several thousand records from more than one receiver is replayed by up to six more host threads, a receiver's
 * buffers to one thread, created when the first such pass is collected and joined by adsb_destroy.
 *
 *   adsb_set_receivers(n)   n = 0: off (default).  ADSB_ERR_BUSY while passes are pending; ADSB_ERR_INVALID for
 *                           n > ADSB_MAX_RECEIVERS and while carry-over is enabled (and adsb_set_carry_over(ctx, 1) is
 *                           ADSB_ERR_INVALID while receivers are on: a buffer's lead-in would have to be the end of its
 *                           own receiver's previous buffer).  Any change of n restarts every receiver from an empty
 *                           filter, as adsb_icao_flush does.  Allocates (n - 1) x 16 KB of host memory for the
 *                           filters, and room for a map of max_chunks entries per pass in flight.  Works on every
 *                           context size.
 *   adsb_get_receivers      n, or ADSB_ERR_INVALID for a null context.
 *   with receivers on       the plain calls (adsb_demod_iq*, submit, the ring, adsb_demodulate2400) mean "every buffer
 *                           is receiver 0": n = 1 is exactly the plain behaviour.  adsb_icao_flush empties EVERY
 *                           receiver's filter.  adsb_shard_scan returns ADSB_ERR_INVALID; adsb_multi_* have no such
 *                           mode.  Error correction (a repair consults the filter of the trial's own receiver), the CU8
 *                           table, signal statistics, profiling, adsb_set_stream and adsb_host_register apply unchanged.
 *   with receivers off      every _rx call, adsb_icao_flush_receiver and adsb_receiver_filter_table return
 *                           ADSB_ERR_INVALID.
 *   an invalid map          (null, or an entry >= n) is ADSB_ERR_INVALID with nothing enqueued and no filter touched.
 *   adsb_icao_flush_receiver(r)  == icao_flush() for receiver r alone.  May be called with passes pending: it applies
 *                           to the passes submitted after it, like adsb_icao_flush (it is recorded against the next
 *                           submission and applied when that pass is collected, in front of its replay).  Host only:
 *                           the device's superset is NOT cleared -- it stays a superset, r's old addresses cost a few
 *                           records that score -1 until an adsb_icao_flush retires the superset.
 *   adsb_receiver_filter_table(r)  table A of receiver r's filter, for inspection.  ADSB_ERR_BUSY while passes are in
 *                           flight.
 *
 * Scoring on the device, per receiver -- opt-in, off by default; with it off nothing observable changes (no launch, no
 * memory, the same adsb_host_replays counts).
 *   adsb_set_receiver_scoring(ctx, enabled)   ADSB_ERR_BUSY while passes are pending, ADSB_ERR_INVALID for a null
 *                           context, ADSB_OK otherwise -- also with receivers off and on a context created with
 *                           max_chunks <= 16: the setting is remembered, and it has no effect where no pass is ever
 *                           ordered on the device (a context of <= 16 buffers, passes of <= 16 buffers, sparse streams).
 *   adsb_get_receiver_scoring   1 / 0, or ADSB_ERR_INVALID for a null context.
 * With receivers on and scoring on, a pass the library would order on the device (a large context, more than 16 buffers,
 * a stream that has left >= 8 trial records per buffer) is scored there too, by kernels of its own that ask "is value v
 * in the filter of THIS BUFFER'S receiver": a set keyed by (receiver, value) holds the filters as they stand before the
 * pass, a table keyed the same way the first trial of the pass that adds each pair.  What comes back is the defining
 * equation above, field for field, signal_level bit for bit, through every _rx call, their _u8 twins,
 * adsb_ring_submit_rx and the plain calls, in every error-correction mode.  The host's filters remain the authority:
 * every pass's additions are applied to them at collect, and the host replays the pass itself (adsb_host_replays)
 * whenever it cannot take the device's result -- a receiver whose table would come within 64 of its 4096 slots, an
 * insertion into a keyed table that ran out of its constant probe bound, a pass behind one the host scored.
 *   footprint               reserved the first time the mode is on together with receivers (in a large context).  Device:
 *                           two keyed sets of 8 x 2^k bytes, 2^k the power of two >= 8192 n_receivers, capped at 2^22
 *                           slots (64 KB each for one receiver, 4 MiB for 64, 32 MiB from 512 on; more than ~2 million
 *                           addresses over all receivers do not fit and leave such passes to the host); per pass in
 *                           flight 4 max_chunks + 4 S bytes and a keyed table the size of the plain one, S the scored
 *                           message slots of adsb_create's footprint (min(4096 + 1024 max_chunks, 262144)).  Pinned
 *                           host: per pass in flight 4 max_chunks + 4 S bytes.  max_chunks = 512, 512 receivers: 64 MiB
 *                           + 4 x 5.2 MB device, 4 x 1.05 MB pinned.
 *   adsb_icao_flush         switches to the other (empty) keyed set, as it does for the one filter: nothing is drained.
 *   adsb_icao_flush_receiver   DRAINS the pipeline while scoring is on: the keyed set cannot forget one receiver, so the
 *                           next pass scored on the device first waits for every pass in flight (their results still
 *                           come from adsb_collect, in order) and rebuilds the set from the host's filters.
 * Not offered: carry-over with receivers (the scan kernel would need a lead-in source per buffer), valid lengths per
 * buffer, receivers in adsb_multi / the shard calls, and adsb_feed. */
#define ADSB_MAX_RECEIVERS 16384
int adsb_set_receivers(adsb_ctx *ctx, uint32_t n_receivers);
int adsb_get_receivers(const adsb_ctx *ctx);
int adsb_icao_flush_receiver(adsb_ctx *ctx, uint32_t receiver);
int adsb_receiver_filter_table(const adsb_ctx *ctx, uint32_t receiver, uint32_t *out4096);
/* adsb_demod_iq, adsb_demod_iq_device, adsb_submit_iq_device and their _u8 twins, with the map */
int adsb_demod_iq_rx(adsb_ctx *ctx, const int16_t *iq_re_im, size_t n_samples, const uint32_t *receiver_of_buffer,
                     adsb_msg *out, size_t cap, size_t *n_out);
int adsb_demod_iq_device_rx(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples,
                            const uint32_t *receiver_of_buffer, adsb_msg *out, size_t cap, size_t *n_out);
int adsb_submit_iq_device_rx(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples,
                             const uint32_t *receiver_of_buffer);
int adsb_demod_iq_rx_u8(adsb_ctx *ctx, const uint8_t *iq_re_im, size_t n_samples, const uint32_t *receiver_of_buffer,
                        adsb_msg *out, size_t cap, size_t *n_out);
int adsb_demod_iq_device_rx_u8(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples,
                               const uint32_t *receiver_of_buffer, adsb_msg *out, size_t cap, size_t *n_out);
int adsb_submit_iq_device_rx_u8(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples,
                                const uint32_t *receiver_of_buffer);
/* adsb_ring_submit with the map of the slot's buffers (a ring of either format): the aggregator's loop -- one slot holds
 * one buffer from each of up to max_chunks receivers */
int adsb_ring_submit_rx(adsb_ctx *ctx, size_t n_samples, const uint32_t *receiver_of_buffer);
/* Host only, no context: the ordered replay with one filter per receiver.  filter_tables: n_receivers x 4096 u32 (table A
 * of receiver r at filter_tables + 4096 r), read and updated.  `records` in any order, chunk = buffer index
 * (< n_buffers, the length of the map; ADSB_ERR_INVALID otherwise, as for a map entry >= n_receivers, with no table
 * touched).  mode: ADSB_FIX_*.  threads <= 1: one walk over the records; threads > 1: the receivers dealt to that many
 * threads.  The same messages and tables whatever `threads`. */
int adsb_replay_records_rx(uint32_t *filter_tables, uint32_t n_receivers, const uint32_t *receiver_of_buffer, size_t n_buffers,
                           adsb_trial *records, size_t n, int mode, int threads, adsb_msg *out, size_t cap, size_t *n_out);
/* Test hooks (results never depend on them).  parallel_min: passes of at least this many trial records, with more than
 * one receiver in them, are replayed by several host threads (0 = the default, 8192); ADSB_ERR_BUSY while passes are
 * pending.  out4: [0] passes replayed per receiver, [1] of them by several threads, [2] times the device's superset was
 * put back from the union of the receivers' filters (overflow fallback, rematch), [3] 0. */
int adsb_selftest_rx_tune(adsb_ctx *ctx, uint32_t parallel_min);
int adsb_selftest_rx_counters(const adsb_ctx *ctx, uint64_t *out4);
int adsb_set_receiver_scoring(adsb_ctx *ctx, int enabled);
int adsb_get_receiver_scoring(const adsb_ctx *ctx);
/* Test hooks of the scoring per receiver (results never depend on them).
 * counters, out4: [0] passes whose device result the host took, [1] passes scored on the device that the host replayed
 * itself all the same (result refused or disowned), [2] rebuilds of the keyed set from the host's filters, [3] passes in
 * which an insertion ran out of probes.
 * tune: the keyed set shrunk to 2^set_lg slots (4 .. 22, never more than it was allocated with) and its probe bound set
 * to probe_max (<= 4096), so that a few hundred addresses reach the out-of-probes path; 0 / 0 restores the defaults
 * (from n_receivers; 64 probes).  ADSB_ERR_BUSY while passes are pending.
 * set_lookup: fills a scratch set of the context's current geometry with `keys` (none may be all ones) through the device
 * function the emit kernel inserts with, answers `queries` through the one the score kernel looks up with: out[i] = 1 / 0
 * for i < n_q, and out[n_q] = the insertions that ran out of probes (`out` holds n_q + 1 words).
 * adsb_rx_set_home: host only, the slot a key's probes start at in a set of 2^set_lg slots (1 <= set_lg <= 32, else 0);
 * key = receiver << 24 | value. */
int adsb_selftest_rx_score_counters(const adsb_ctx *ctx, uint64_t *out4);
int adsb_selftest_rx_score_tune(adsb_ctx *ctx, uint32_t set_lg, uint32_t probe_max);
int adsb_selftest_rx_set_lookup(adsb_ctx *ctx, const uint64_t *keys, size_t n_keys, const uint64_t *queries, size_t n_q,
                                uint32_t *out);
uint32_t adsb_rx_set_home(uint64_t key, uint32_t set_lg);

/* ---------------------------------------------------------------------------------------------------------
 * Receiver seams -- carry-over with receivers on.  Opt-in, off by default; with it off nothing changes: no launch, no
 * allocation.  This mode is the way to get carry-over with many receivers: adsb_set_carry_over itself stays
 * ADSB_ERR_INVALID while receivers are on, as the section above says.
 *
 * Without it every buffer of every receiver starts from a zero lead-in, and a preamble that begins in the last 326
 * samples of a receiver's buffer is never tried (326 of every 131072 positions).  With it:
 *
 * Definition.  The sentence that defines the _rx calls, with one change: feed receiver r's buffers, one adsb_demod_iq
 * call per buffer, to a plain context r of its own THAT HAS adsb_set_carry_over(ctx, 1); relabel every message's `chunk`
 * with b; merge in ascending (chunk, j).  That merged list is what every _rx call, its _u8 twin, submit / collect,
 * adsb_ring_submit_rx and the plain IQ calls ("every buffer is receiver 0") return, field for field and signal_level bit
 * for bit, in every error-correction mode, and adsb_receiver_filter_table(r) equals context r's table slot for slot.
 * `j` stays the index into MagnitudeBuffer.data: a frame that starts in the lead-in has j < 326, as under
 * adsb_set_carry_over.  A receiver's stream is CS16 inside the library: CS16 and CU8 buffers may alternate.  A short
 * last buffer of n < 326 samples leaves its receiver's carry as the last 326 samples of (old carry ++ buffer).
 *
 * How: a trial at position j reads data[j .. j+290] and nothing else, so a buffer's lead-in decides the trials at
 * j < 326 and no others.  The pass's scan runs unchanged; kernels of their own gather a lead-in per buffer (the
 * receiver's carry, or the end of the receiver's previous buffer in the same pass), try those 326 positions per buffer in
 * front of the scan -- what they learn is in the address superset before the pass's match reads it -- and match their
 * address/parity trials behind the pass's last kernel.  The host drops the pass's own records with j < 326 and replays
 * the seam's records in their place, buffer by buffer against the receiver's filter as before.  All passes of a context
 * in this mode run on one scan stream, ordered by it (as under adsb_set_carry_over).
 *
 *   adsb_set_receiver_carry(ctx, enabled)   ADSB_ERR_BUSY while passes are pending; ADSB_ERR_INVALID for a null context,
 *                           with receivers off, and while adsb_set_receiver_scoring is on (and
 *                           adsb_set_receiver_scoring(ctx, 1) is ADSB_ERR_INVALID while this mode is on: seam trials are
 *                           scored by the host).  Enabling, disabling and any change of adsb_set_receivers restart every
 *                           receiver's stream with nothing before its next buffer; adsb_set_receivers(ctx, 0) turns the
 *                           mode off.  adsb_icao_flush and adsb_icao_flush_receiver touch filters only.
 *   adsb_get_receiver_carry   1 / 0, or ADSB_ERR_INVALID for a null context.
 *   adsb_receiver_carry_reset(ctx, r)   receiver r (or all, ADSB_RX_ALL) reconnected: nothing precedes its next buffer.
 *                           Ordered between the submissions before and after it; never ADSB_ERR_BUSY;
 *                           ADSB_ERR_INVALID for r >= n and with the mode off.
 *   unchanged               adsb_demodulate2400 (the caller's magnitudes), the signal statistics (a lead-in is not
 *                           counted), and everything with the mode off.
 *   footprint               reserved by the enable.  Device: 1312 bytes per receiver; per pass in flight 1312 max_chunks
 *                           bytes of lead-ins and a seam list of S x 32 bytes, S = min(max(2048, 64 max_chunks), 65536).
 *                           Pinned host: per pass in flight 16 max_chunks + S x 32 bytes.  A full seam list or record
 *                           block makes the library redo that pass's seam step in pieces sized for the worst case (326 x 5
 *                           records a buffer; 417 KB more pinned memory, reserved then): nothing is lost.
 * Not part of this mode: valid lengths per buffer, seam trials scored on the device, and seams in adsb_multi and
 * adsb_feed.
 * Test hooks (results never depend on them).  tune: the seam list and record block of the passes submitted from now on
 * hold list_cap entries (0 = the default; never more than was reserved); ADSB_ERR_BUSY while passes are pending.
 * counters, out4: [0] passes with a seam step, [1] seam records handed to the replay, [2] records of the pass itself
 * dropped for j < 326, [3] seam steps redone after an overflow. */
#define ADSB_RX_ALL 0xFFFFFFFFu
int adsb_set_receiver_carry(adsb_ctx *ctx, int enabled);
int adsb_get_receiver_carry(const adsb_ctx *ctx);
int adsb_receiver_carry_reset(adsb_ctx *ctx, uint32_t receiver);
int adsb_selftest_rx_seam_tune(adsb_ctx *ctx, uint32_t list_cap);
int adsb_selftest_rx_seam_counters(const adsb_ctx *ctx, uint64_t *out4);

/* ---------------------------------------------------------------------------------------------------------
 * Receiver seams, scored on the device -- adsb_set_receiver_carry AND adsb_set_receiver_scoring, which refuse each other
 * as single modes (above: each says why), as one mode with an entry point of its own.  Opt-in, off by default; with it
 * off nothing changes: no launch, no allocation, the two single setters behave as documented.
 *
 * Definition.  The "Receiver seams" definition, unchanged: the list equals one plain context WITH carry-over per receiver,
 * relabelled and merged in (chunk, j), field for field, signal_level bit for bit, every receiver's filter table slot for
 * slot, in all three error-correction modes, through every _rx call, its _u8 twin, submit / collect,
 * adsb_ring_submit_rx and the plain IQ calls.  The only difference from adsb_set_receiver_carry alone is who scores: a
 * pass the library orders on the device (a large context, more than 16 buffers, a stream that has left >= 8 trial records
 * per buffer) takes its result from the device.
 *
 * How: behind the pass's seam match, on the score stream, kernels of their own merge the pass's seam records into the
 * records kernel's ordered hits and drop the pass's own hits at j < 326 -- into a second set of score arrays, which the
 * keyed score kernels of adsb_set_receiver_scoring then take for the pass's, unchanged.  The seam records reach that merge
 * through a mirror in device memory.  A pass whose seam list or record block overflowed, or whose merged hits outnumber
 * the score arrays, declares itself unscored on the device: the host then redoes the seam step in pieces and replays, as
 * under adsb_set_receiver_carry, and the next pass scored on the device rebuilds the keyed set.  Every other pass of the
 * mode (small contexts, passes of <= 16 buffers, sparse streams, caller-supplied magnitudes) is the host's, seams
 * included, exactly as under adsb_set_receiver_carry.
 *
 *   adsb_set_receiver_carry_scoring(ctx, enabled)   ADSB_ERR_BUSY while passes are pending; ADSB_ERR_INVALID for a null
 *                           context and with receivers off; ADSB_OK on every context size (a context that never orders a
 *                           pass on the device keeps host-scoring its seam passes).  Enabling may come from any state of
 *                           the two single modes, reserves what both reserve and the footprint below, and restarts every
 *                           receiver's stream, as enabling adsb_set_receiver_carry does; afterwards
 *                           adsb_get_receiver_carry and adsb_get_receiver_scoring both return 1.  While it is on,
 *                           adsb_set_receiver_carry and adsb_set_receiver_scoring return ADSB_OK for the value in effect
 *                           (1) and ADSB_ERR_INVALID for a change.  Disabling turns both off and releases the seams' and
 *                           the merge's storage (the keyed sets stay reserved, as after adsb_set_receiver_scoring(ctx, 0));
 *                           adsb_set_receivers(ctx, 0) turns the mode off; any other change of the receiver count
 *                           restarts every stream and re-sizes both footprints.
 *   adsb_get_receiver_carry_scoring   1 / 0, or ADSB_ERR_INVALID for a null context.
 *   unchanged               adsb_receiver_carry_reset, adsb_icao_flush (switches to the empty keyed set) and
 *                           adsb_icao_flush_receiver (still DRAINS while scoring is on) behave as documented for the
 *                           single modes.
 *   footprint               on top of both single modes', in a context that scores on the device.  Device, per pass in
 *                           flight: 52 S bytes of merged score arrays (S the scored message slots of adsb_create's
 *                           footprint), a mirror of the seam's record block (32 bytes x the seam list's entries) and 228
 *                           max_chunks bytes of work arrays: about 1.4 MB at max_chunks = 20, about 15 MB at 512.  Pinned
 *                           host: 256 bytes per pass in flight.
 *   counters                a merged pass whose device result is taken leaves adsb_selftest_rx_seam_counters' records,
 *                           dropped and redone where they were: the host neither merges nor replays its seam records
 *                           ([0], passes with a seam step, counts it as before).
 * Test hooks (results never depend on them).  counters, out4: [0] passes with a device-side seam merge, [1] seam records
 * merged on the device, [2] own hits dropped on the device for j < 326, [3] merged passes that declared themselves
 * unscored (seam overflow, or more merged hits than the score arrays hold).  Counted at collect for every pass whose merge
 * ran, also one whose device result is then refused or disowned.  adsb_selftest_reservations: how many
 * reservations (device blocks, pinned blocks, events) the context's owner holds now. */
int adsb_set_receiver_carry_scoring(adsb_ctx *ctx, int enabled);
int adsb_get_receiver_carry_scoring(const adsb_ctx *ctx);
int adsb_selftest_rx_seam_score_counters(const adsb_ctx *ctx, uint64_t *out4);
uint64_t adsb_selftest_reservations(const adsb_ctx *ctx);

/* ---------------------------------------------------------------------------------------------------------
 * Decimation -- IQ sampled at an integer multiple of 2.4 MS/s.  Every entry point above takes IQ at exactly 2.4 MS/s;
 * a HackRF, bladeRF, USRP or Airspy runs at 4.8, 9.6, 12, 19.2 or 24 MS/s.  An adsb_decim is a stateful, exact-integer
 * FIR decimator by an integer factor D that runs on the device in front of the scan, in a kernel of its own: its output
 * is ordinary CS16 in device memory, which every call above takes.  Nothing else changes.
 *
 * Definition.  x[m], m = 0, 1, ..., is the input counted from adsb_decim_create or adsb_decim_reset, complex, `re` then
 * `im` as in the CS16 calls; x[m] = 0 for m < 0.  With taps h[0..T-1] (int16) and shift s, for n = 0, 1, ... and for re and
 * im separately:
 *     acc  = sum over k of h[k] * x[n D - k]
 *     y[n] = clamp((acc + r) >> s, -32768, 32767),   r = 1 << (s - 1), or 0 when s == 0,   >> arithmetic (a half rounds up)
 * y is CS16 {re, im}.  D in 2..16, 1 <= T <= 512, s in 0..16, sum |h[k]| <= 65534 (an int32 accumulator then never wraps);
 * anything else is ADSB_ERR_INVALID.
 * A call with n_in inputs, P inputs having been consumed before it, produces exactly the y[n] with P <= n D < P + n_in:
 * ceil((P + n_in) / D) - ceil(P / D) of them, possibly none.  The cut is invisible: the concatenated outputs of any
 * cutting of a stream into calls -- calls of no input and calls shorter than T - 1 included -- equal the one-call result
 * bit for bit.  The decimator keeps the last T - 1 inputs (on the device, in two buffers that take turns) and P (on the
 * host: counts are host arithmetic, no call synchronises to learn one).
 * 8-bit input (ADSB_DECIM_8BIT): byte b means T8[b], T8 the context's table at the time of the call (adsb_set_u8_table;
 * T_soapy by default; a HackRF's CS8 is T8[b] = (int8_t)b << 8).  The bytes are widened as they are loaded and the history
 * is kept widened, so a stream may alternate the formats; x[m < 0] is zero by position, not T8[0].  (adsb_set_u8_table does
 * not wait for decimator calls still running: synchronise the stream before changing the table under them.)
 *
 *   adsb_decim_create        a decimator on the context's device.  Destroy it before the context.
 *   adsb_decim_reset         the stream starts over (P = 0, zero history); ordered on the stream like a run
 *   adsb_decim_out_count     host only: how many outputs the next run of n_in inputs would produce
 *   adsb_decim_run_device    device memory to device memory (both 16-byte aligned, not overlapping).  Enqueues on the stream
 *                            the context orders its input behind -- the caller's after adsb_set_stream, else the context's
 *                            own -- and returns without waiting; *n_out is known at once.  The next pass submitted on the
 *                            context waits for it, so the asynchronous form of the feature is
 *                                adsb_decim_run_device(d, fmt, in, n_in, y, cap, &n);  adsb_submit_iq_device(ctx, y, n);
 *                            with no synchronisation in between.  out_cap too small: ADSB_ERR_CAPACITY with the required
 *                            count in *n_out; nothing is consumed and the state does not change.  Never ADSB_ERR_BUSY:
 *                            the decimator does not care about pending passes.
 *   adsb_decim_demod_iq      blocking, host input of any length: exactly what adsb_demod_iq returns on the y this call's
 *                            input decimates to -- buffers are cut every 131072 OUTPUT samples of the call, the last may
 *                            be short, `chunk` counts over the call; the filter persists.  Works in pieces of whole
 *                            output buffers, min(max_chunks, 16) of them at most, through staging the decimator allocates
 *                            on first use (at most b D + 4 bytes per output sample of a piece, b the bytes of an input
 *                            sample: 8 for CF32, 4 for CS16, 2 for 8-bit and REAL16 -- "Sample formats") and frees in
 *                            adsb_decim_destroy.  ADSB_ERR_CAPACITY, adsb_fetch_messages, ADSB_ERR_BUSY and every context
 *                            mode (error correction, signal statistics, carry-over) are adsb_demod_iq's: the pass
 *                            underneath is the ordinary one.
 *   adsb_decim_default_taps  host only: a Hamming-windowed sinc with its cutoff at 1.2 MHz, 8 D + 1 taps, symmetric, scaled
 *                            to sum 2^15 (shift 15; sum |h| <= 65534).  Computed in double through libm: a property, not
 *                            bits.  `cap` too small: ADSB_ERR_CAPACITY with the count in *n_taps.
 * After a HIP failure the decimator's state is undefined until adsb_decim_reset. */
typedef struct adsb_decim adsb_decim;
#define ADSB_DECIM_CS16 0
#define ADSB_DECIM_8BIT 1
ADSB_MUST_CHECK int adsb_decim_create(adsb_ctx *ctx, uint32_t factor, const int16_t *taps, uint32_t n_taps, uint32_t shift,
                                      adsb_decim **out);
extern void adsb_decim_destroy(adsb_decim *d);
ADSB_MUST_CHECK int adsb_decim_reset(adsb_decim *d);
ADSB_MUST_CHECK int adsb_decim_out_count(const adsb_decim *d, size_t n_in, size_t *n_out);
ADSB_MUST_CHECK int adsb_decim_run_device(adsb_decim *d, int format, const void *device_in, size_t n_in, void *device_out_cs16,
                                          size_t out_cap, size_t *n_out);
ADSB_MUST_CHECK int adsb_decim_demod_iq(adsb_decim *d, int format, const void *host_iq, size_t n_in, adsb_msg *out, size_t cap,
                                        size_t *n_out);
ADSB_MUST_CHECK int adsb_decim_default_taps(uint32_t factor, int16_t *taps, size_t cap, uint32_t *n_taps, uint32_t *shift);
/* Host only, for the tests: the outputs one workgroup of the decimating kernel takes. */
uint32_t adsb_decim_selftest_tile(void);

/* ---------------------------------------------------------------------------------------------------------
 * Resampling -- IQ sampled at a rate that is no integer multiple of 2.4 MS/s: an Airspy at 2.5, 3, 6 or 10 MS/s, a
 * HackRF at 8, 10 or 20 MS/s, an RTL-SDR at 2.0, 2.56 or 3.2 MS/s, a USRP B2xx at 12.5 MS/s.  An adsb_resamp is a
 * stateful, exact-integer polyphase FIR resampler by a ratio L / M (`up` / `down`) that runs on the device in front of
 * the scan, in a kernel of its own beside the decimator's: its output is ordinary CS16 in device memory, which every call
 * above takes.  Nothing else changes.
 *
 * Definition.  An adsb_resamp turns input at rate f into output at rate f L / M.  x[m], m = 0, 1, ..., is the input
 * counted from adsb_resamp_create or adsb_resamp_reset, complex, `re` then `im`; x[m] = 0 for m < 0.  With prototype taps
 * h[0..T-1] (int16) and shift s, for n = 0, 1, ... and for re and im separately:
 *     p = (n M) mod L,   q = floor(n M / L)
 *     acc  = sum over j >= 0 with p + j L < T of  h[p + j L] * x[q - j]
 *     y[n] = clamp((acc + r) >> s, -32768, 32767),   r = 1 << (s - 1), or 0 when s == 0,   >> arithmetic (a half rounds up)
 * -- zero-stuffing by L, the FIR h, then keeping every M-th sample, with the zero products left out.  K = ceil(T / L) is
 * the most taps one output uses.  Accepted: 1 <= L <= 128 and 1 <= M <= 128 with gcd(L, M) = 1, L <= 2 M (upsampling
 * beyond 2 x has no use here), M <= 16 L (the decimator's reach), 1 <= T <= 4096 with K <= 512, s in 0..16, and for every
 * phase p the sum over j of |h[p + j L]| <= 65534 (an int32 accumulator then never wraps); anything else is
 * ADSB_ERR_INVALID.  With L = 1 the definition is the decimator's with D = M; L = M = 1 is a plain FIR.
 * Counts.  A call of n_in inputs, P inputs having been consumed before it, produces exactly the y[n] whose newest input
 * lies in the call, P <= floor(n M / L) < P + n_in: the n with
 *     ceil(P L / M) <= n < ceil((P + n_in) L / M)
 * possibly none.  The cut is invisible: the concatenated outputs of any cutting of a stream into calls -- calls of no
 * input and calls shorter than K - 1 included -- equal the one-call result bit for bit.  The resampler keeps the last
 * K - 1 inputs (on the device, widened, in two buffers that take turns) and P (on the host: counts are 64-bit host
 * arithmetic, no call synchronises to learn one).
 * 8-bit input (ADSB_DECIM_8BIT, or its alias ADSB_RESAMP_8BIT) works as in the decimator: byte b means T8[b], T8 the
 * context's table at the time of the call; the bytes are widened as they are loaded and the history is kept widened, so a
 * stream may alternate the formats; x[m < 0] is zero by position, not T8[0].  (Synchronise the stream before changing the
 * table under calls still running.)
 *
 *   adsb_resamp_create          a resampler on the context's device.  Destroy it before the context.
 *   adsb_resamp_reset           the stream starts over (P = 0, zero history); ordered on the stream like a run
 *   adsb_resamp_out_count       host only: how many outputs the next run of n_in inputs would produce
 *   adsb_resamp_run_device      device memory to device memory (both 16-byte aligned, not overlapping), as
 *                               adsb_decim_run_device: enqueues on the stream the context orders its input behind and
 *                               returns without waiting; *n_out is known at once; the next pass submitted on the context
 *                               waits for it.  out_cap too small: ADSB_ERR_CAPACITY with the required count in *n_out;
 *                               nothing is consumed and the state does not change.  Never ADSB_ERR_BUSY.
 *   adsb_resamp_demod_iq        blocking, host input of any length: exactly what adsb_demod_iq returns on the y this call's
 *                               input resamples to -- buffers are cut every 131072 OUTPUT samples of the call, the last
 *                               may be short, `chunk` counts over the call; the filter persists.  Works in pieces of whole
 *                               output buffers, min(max_chunks, 16) of them at most, through staging the resampler
 *                               allocates on first use and frees in adsb_resamp_destroy.  (Where L > M two consecutive
 *                               outputs can share their newest input; a piece may then produce one output more than its
 *                               buffers hold, which is carried to the front of the next piece.)  ADSB_ERR_CAPACITY,
 *                               adsb_fetch_messages, ADSB_ERR_BUSY and every context mode are adsb_demod_iq's: the pass
 *                               underneath is the ordinary one.
 *   adsb_resamp_default_taps    host only: a Hamming-windowed sinc over the zero-stuffed rate with its cutoff at half the
 *                               lower of the two rates, 8 max(L, M) + 1 taps, symmetric, scaled so that the prototype
 *                               sums to L 2^14 -- every phase to about 2^14 -- with shift 14 (at 2^15 the centre tap would
 *                               not fit an int16 where L > M).  Computed in double through libm: a property, not bits.
 *                               `cap` too small: ADSB_ERR_CAPACITY with the count in *n_taps.
 *   adsb_resamp_ratio_for_rate  host only: the ratio that brings rate_hz to 2.4 MS/s, up = 2 400 000 / g and
 *                               down = rate_hz / g with g their greatest common divisor; ADSB_ERR_INVALID (with the
 *                               terms still written) where the ratio is outside the limits above.
 *   adsb_resamp_plan            host only, no handle: the count formula above -- the first output ceil(consumed L / M)
 *                               and the number of outputs of a call of n_in inputs behind `consumed` (both < 2^56).
 * After a HIP failure the resampler's state is undefined until adsb_resamp_reset. */
typedef struct adsb_resamp adsb_resamp;
#define ADSB_RESAMP_CS16 ADSB_DECIM_CS16
#define ADSB_RESAMP_8BIT ADSB_DECIM_8BIT
ADSB_MUST_CHECK int adsb_resamp_create(adsb_ctx *ctx, uint32_t up, uint32_t down, const int16_t *taps, uint32_t n_taps,
                                       uint32_t shift, adsb_resamp **out);
extern void adsb_resamp_destroy(adsb_resamp *r);
ADSB_MUST_CHECK int adsb_resamp_reset(adsb_resamp *r);
ADSB_MUST_CHECK int adsb_resamp_out_count(const adsb_resamp *r, size_t n_in, size_t *n_out);
ADSB_MUST_CHECK int adsb_resamp_run_device(adsb_resamp *r, int format, const void *device_in, size_t n_in,
                                           void *device_out_cs16, size_t out_cap, size_t *n_out);
ADSB_MUST_CHECK int adsb_resamp_demod_iq(adsb_resamp *r, int format, const void *host_iq, size_t n_in, adsb_msg *out,
                                         size_t cap, size_t *n_out);
ADSB_MUST_CHECK int adsb_resamp_default_taps(uint32_t up, uint32_t down, int16_t *taps, size_t cap, uint32_t *n_taps,
                                             uint32_t *shift);
ADSB_MUST_CHECK int adsb_resamp_ratio_for_rate(uint32_t rate_hz, uint32_t *up, uint32_t *down);
ADSB_MUST_CHECK int adsb_resamp_plan(uint32_t up, uint32_t down, uint64_t consumed, uint64_t n_in, uint64_t *first_n,
                                     uint64_t *n_out);
/* Host only, for the tests: the outputs one workgroup of the resampling kernel takes at this ratio (0: not a ratio). */
uint32_t adsb_resamp_selftest_tile(uint32_t up, uint32_t down);

/* ---------------------------------------------------------------------------------------------------------
 * Frequency shift -- offset-tuned IQ.  A HackRF, bladeRF, Airspy or USRP is a zero-IF receiver: its DC spike and LO
 * leakage sit exactly on the tuned frequency, and the demodulator works on magnitudes.  Such a radio is therefore tuned a
 * megahertz or two beside 1090 MHz at its higher rate and the signal is mixed back digitally; the decimating low-pass
 * then removes the spike, which now lies beside the band.  A decimator or a resampler may carry a MIXER that does this on
 * the device, on the samples' way into the filter: no kernel of its own, no second pass over the high-rate input.
 *
 * Definition.  A mixer is a table w[0..N-1] of int16 pairs (c, s), 1 <= N <= ADSB_MIX_MAX_PERIOD (256), every
 * |c|, |s| <= 32767 (the value -32768 is ADSB_ERR_INVALID).  With a mixer set, the x[m] in the decimator's or resampler's
 * definition is replaced by x'[m]; m is the sample's index in the stream counted from create or reset, the P the handle
 * keeps:
 *     t   = m mod N
 *     re' = clamp((x.re * c[t] - x.im * s[t] + 8192) >> 14, -32768, 32767)
 *     im' = clamp((x.re * s[t] + x.im * c[t] + 8192) >> 14, -32768, 32767)      >> arithmetic (a half rounds up)
 * -- x[m] (c + i s) / 2^14.  Everything after it is unchanged: taps, shift, counts, and "the cut is invisible", which now
 * covers the mixer's phase too.  x'[m] = 0 for m < 0.  8-bit input is widened through the context's table first, then
 * mixed.  The history holds mixed samples, so the mixer may be set, changed or cleared between calls; the table is applied
 * by absolute m, whatever was set before.  The int32 accumulator cannot wrap: 2 * 32768 * 32767 + 8192 < 2^31.  With
 * amplitude 2^14 and the shift of 14 a table entry (16384, 0) is the identity, and the tables of N = 1, 2, 4 are exact
 * rotations by 0, 180 and 90 degrees.
 *
 *   adsb_mix_set_decim   }  cs_pairs: `period` pairs {c, s}.  Ordered on the stream like *_reset: applies to the inputs
 *   adsb_mix_set_resamp  }  consumed after the call.  The table is copied during the call.  NULL with period 0 turns the
 *                             mixer off.  An invalid table is ADSB_ERR_INVALID and changes nothing.  Never ADSB_ERR_BUSY.
 *   adsb_mix_get_decim   }  the period; 0 when the mixer is off
 *   adsb_mix_get_resamp  }
 *                          (All six calls carry the adsb_mix_ prefix: the adsb_decim_* and adsb_resamp_* families are
 *                          what they were.)
 *   adsb_mix_table         host only: the table of a shift by k / N cycles per sample, c[t] = lround(16384 cos(2 pi k t / N))
 *                          and s likewise with sin.  Computed in double through libm: a property, not bits -- but whole
 *                          quarter turns are exact, so the tables of N = 1, 2, 4 are.  `cap` (in pairs) below `period`:
 *                          ADSB_ERR_CAPACITY.
 *   adsb_mix_for_shift     host only: the table terms for a stream at 2.4 MS/s x down / up (a decimator is (1, D); both
 *                          terms 1..128) whose spectrum is to be moved by shift_hz, signed: a radio tuned 2.4 MHz BELOW
 *                          1090 MHz sees the signal 2.4 MHz above its centre and passes -2 400 000.
 *                          k / N = shift_hz up / (2 400 000 down), reduced, k taken mod N into 0..N-1.  ADSB_ERR_INVALID
 *                          (with the terms still written) where N > 256.
 * Keep |shift_hz| well inside the stopband of the filter behind the mixer: the spike ends up |shift_hz| from the centre. */
#define ADSB_MIX_MAX_PERIOD 256u
ADSB_MUST_CHECK int adsb_mix_set_decim(adsb_decim *d, const int16_t *cs_pairs, uint32_t period);
ADSB_MUST_CHECK int adsb_mix_set_resamp(adsb_resamp *r, const int16_t *cs_pairs, uint32_t period);
extern uint32_t adsb_mix_get_decim(const adsb_decim *d);
extern uint32_t adsb_mix_get_resamp(const adsb_resamp *r);
ADSB_MUST_CHECK int adsb_mix_table(uint32_t k, uint32_t period, int16_t *cs_pairs, size_t cap);
ADSB_MUST_CHECK int adsb_mix_for_shift(uint32_t up, uint32_t down, int32_t shift_hz, uint32_t *k, uint32_t *period);

/* ---------------------------------------------------------------------------------------------------------
 * Sample formats -- complex float32 and real int16 input.  CS16 and 8-bit pairs are two of the layouts the radios above
 * produce.  Complex float32 (CF32) is the stream format of SoapySDR applications and GNU Radio file sinks, what gqrx and
 * SigMF `cf32_le` record and what `airspy_rx -t 0` and UHD `fc32` deliver; an Airspy R2 or Mini samples REAL values
 * (`airspy_rx -t 3`: int16 at 20 or 12 MS/s, the band at a quarter of the sample rate).  A decimator or a resampler reads
 * both: adsb_decim_run_device, adsb_decim_demod_iq, adsb_resamp_run_device and adsb_resamp_demod_iq take the two formats
 * below as they take CS16 and 8-bit, signatures and semantics unchanged.  The sample is converted to CS16 on the device
 * between the load and the mixer: no kernel of its own, no second pass over the input.
 *
 * Definition.  The converted sample replaces x[m] in the decimator's and the resampler's definitions; the mixer, taps,
 * shift, counts and "the cut is invisible" follow unchanged.
 *   ADSB_DECIM_CF32    8 bytes per sample: float32 re, float32 im, little-endian.  Each component x means q(x), with the
 *                      handle's scale g (32768.0f by default):
 *                          t    = x * g        one IEEE binary32 multiply, round to nearest even, contracted with nothing
 *                          q(x) = 0                                        where t is a NaN
 *                          q(x) = clamp(rint(t), -32768, 32767)            otherwise: ties to even, +-inf to the rails
 *                      A subnormal x gives 0 whether or not the device flushes it: 2^-126 * 2^31 rounds to 0.  So numpy's
 *                          np.rint(x.astype(np.float32) * np.float32(g)), NaN mapped to 0, clipped to -32768 .. 32767
 *                      is q bit for bit, with no tolerance.
 *   ADSB_DECIM_REAL16  2 bytes per sample: one int16 r; x[m] = (r[m], 0).
 * As for 8-bit, a sample outside the call is zero by position: x[m < 0] is zero and so is whatever lies behind the end of
 * the call's input -- the int16 behind an odd number of REAL16 samples, which the rounded-up load does fetch, never
 * reaches the filter.  The history holds converted (and mixed) CS16, so one stream may alternate all four formats from
 * call to call.
 * Sizes.  Device input is 16-byte aligned, as for the other formats.  adsb_*_demod_iq stages 8, 4, 2 or 2 bytes per input
 * sample for CF32, CS16, 8-bit and REAL16: at most that times D (or M / L) plus 4 bytes per output sample of a piece.
 *
 *   adsb_fmt_set_scale_decim   }  g, finite with 0 < g <= 2^31; anything else is ADSB_ERR_INVALID and changes nothing.
 *   adsb_fmt_set_scale_resamp  }  Host state that travels in each launch's parameters: it applies to the calls made after
 *                                 the setter, is never ADSB_ERR_BUSY and means nothing to the other three formats.
 *   adsb_fmt_get_scale_decim   }  g; 0 for NULL
 *   adsb_fmt_get_scale_resamp  }
 *                                 (The four calls carry the adsb_fmt_ prefix: the adsb_decim_* and adsb_resamp_* families
 *                                 gain no function.)
 * Recipes.
 *   CF32 already at 2.4 MS/s   a 1/1 resampler with the single tap 1 and shift 0 -- "L = M = 1 is a plain FIR" with
 *                              K = 1: adsb_resamp_create(ctx, 1, 1, &one, 1, 0, &r), then adsb_resamp_demod_iq(r,
 *                              ADSB_RESAMP_CF32, ...) is adsb_demod_iq on q of the input.
 *   Airspy R2 raw, 20 MS/s     REAL16 through a 3/25 resampler with the mixer adsb_mix_table(3, 4), the exact rotation that
 *                              brings the band at +fs/4 to 0:  adsb_feed --format s16real --resample 3/25 --shift -5000000
 *   Airspy Mini raw, 12 MS/s   REAL16 through a decimator with D = 5 and the same table:
 *                                                              adsb_feed --format s16real --decimate 5 --shift -3000000
 * Not here: exploiting the zero imaginary part, Airspy's unsigned and packed 12-bit real formats, real float32, and float
 * input to the scan's own entry points. */
#define ADSB_DECIM_CF32   2   /* 8 bytes per sample: f32 re, f32 im, little-endian */
#define ADSB_DECIM_REAL16 3   /* 2 bytes per sample: one int16 r; x[m] = (r[m], 0) */
#define ADSB_RESAMP_CF32   ADSB_DECIM_CF32
#define ADSB_RESAMP_REAL16 ADSB_DECIM_REAL16
ADSB_MUST_CHECK int adsb_fmt_set_scale_decim(adsb_decim *d, float scale);
ADSB_MUST_CHECK int adsb_fmt_set_scale_resamp(adsb_resamp *r, float scale);
extern float adsb_fmt_get_scale_decim(const adsb_decim *d);
extern float adsb_fmt_get_scale_resamp(const adsb_resamp *r);

/* ---------------------------------------------------------------------------------------------------------
 * Resampler banks -- many resampler streams in one launch.  A pass of many receivers ("Many receivers, one pass") takes
 * one full 2.4 MS/s buffer per receiver, all in one device allocation.  Where the receivers' radios run at another rate
 * each needs a resampler, and R adsb_resamp handles are R calls of two launches each, one behind the other, every grid a
 * fraction of the device.  An adsb_bank is N independent streams of one ratio and one filter that ONE call advances by
 * one launch of the resampling kernel (and one of the history kernel), whatever N.
 *
 * Definition.  A bank is N streams, 1 <= N <= ADSB_MAX_RECEIVERS, that share (up, down, taps, n_taps, shift) -- with
 * exactly the limits of adsb_resamp_create -- one mixer table (off by default) and one CF32 scale (32768 by default).
 * Stream i of a bank is, bit for bit and count for count, an adsb_resamp that was created with those arguments, was
 * given that mixer table and scale, and was fed the calls that named stream i, in order.  Each stream has its own P
 * (inputs consumed) and its own K - 1 inputs of history; the mixer is applied by the stream's own P; the output phase is
 * the stream's own.  A call that does not name a stream leaves it untouched.  Nothing else is new: "Resampling",
 * "Frequency shift" and "Sample formats" are the specification.
 *
 *   adsb_bank_create      a bank on the context's device.  Destroy it before the context.  Device memory: two histories
 *                         of 2 KB per stream, and four blocks of 64 bytes per stream for the calls' descriptors.
 *   adsb_bank_destroy     waits for what the bank put on the stream, then frees it
 *   adsb_bank_streams     N; 0 for NULL
 *   adsb_bank_reset       stream i, or every stream with ADSB_BANK_ALL, starts over (P = 0, zero history); ordered on
 *                         the stream like a run
 *   adsb_bank_consumed    host only: the stream's P
 *   adsb_bank_out_count   host only: how many outputs the stream's next run of n_in inputs would produce
 *   adsb_bank_inputs_for  host only: the fewest inputs behind the stream's P that give at least n_out_wanted outputs, in
 *                         *n_in, and how many they give, in *n_out_made: n_out_wanted, or one more where L > M (two
 *                         consecutive outputs can share their newest input).  0 wanted: 0 and 0.  This is how a caller
 *                         cuts each receiver's input so that its run fills exactly one 131072-sample buffer.
 *   adsb_bank_run_device  one `format` for the call (ADSB_DECIM_CS16, _8BIT, _CF32 or _REAL16; 8-bit through the
 *                         context's table); run r advances streams[r] by n_in[r] inputs from device_in[r] and writes
 *                         n_out[r] CS16 samples to device_out_cs16[r] -- normally the 131072-sample slots of the one
 *                         allocation the _rx pass then takes.  Device memory to device memory, every pointer 16-byte
 *                         aligned, nothing overlapping.  Enqueues on the stream the context orders its input behind, as
 *                         adsb_resamp_run_device does, and returns without waiting; every n_out[r] is known at once; the
 *                         next pass submitted on the context waits for it.  The arrays are read during the call.
 *                         ADSB_ERR_INVALID -- nothing is enqueued and no stream changes -- for a NULL handle or array, a
 *                         bad format, n_runs > N, streams[r] >= N, a stream named twice in one call, a pointer that is
 *                         not 16-byte aligned, a NULL input with n_in[r] > 0 and a NULL output with n_out[r] > 0.
 *                         ADSB_ERR_CAPACITY if any n_out[r] > out_cap[r]: every n_out[r] is still written and no stream
 *                         of the call consumes anything.  A run of no input does nothing, and so does a call of no
 *                         runs.  Never ADSB_ERR_BUSY.  A call's descriptors travel through one of
 *                         adsb_bank_selftest_depth() blocks used in rotation, each guarded by an event behind the launch
 *                         that reads it: a call that finds its block still in flight waits for that launch; it does not
 *                         fail.
 *   adsb_bank_set_mixer   adsb_mix_set_resamp's rules, for the one table every stream shares (each at its own phase)
 *   adsb_bank_get_mixer   the period; 0 when the mixer is off
 *   adsb_bank_set_scale   adsb_fmt_set_scale_resamp's rules
 *   adsb_bank_get_scale   g; 0 for NULL
 * Cost of uneven runs.  The launch's grid is (tiles of the call's LONGEST run) x (runs with input): a workgroup whose
 * tile lies past its own run's last output returns at once, but it is still scheduled.  A call whose runs are about
 * equal -- one buffer per receiver, the expected use -- wastes nothing; a call of one long and many short runs launches
 * mostly empty workgroups and is better split in two.  A bank with L = 1 covers integer decimation.
 * Not here: a blocking host-pointer *_demod_iq form for banks; per-stream ratios, taps or mixer tables (use one bank per
 * ratio); banks in adsb_feed or adsb_multi; a bank form of adsb_decim.
 * After a HIP failure the bank's state is undefined until adsb_bank_reset(bank, ADSB_BANK_ALL). */
typedef struct adsb_bank adsb_bank;
#define ADSB_BANK_ALL 0xFFFFFFFFu
ADSB_MUST_CHECK int adsb_bank_create(adsb_ctx *ctx, uint32_t n_streams, uint32_t up, uint32_t down, const int16_t *taps,
                                     uint32_t n_taps, uint32_t shift, adsb_bank **out);
extern void adsb_bank_destroy(adsb_bank *b);
extern uint32_t adsb_bank_streams(const adsb_bank *b);
ADSB_MUST_CHECK int adsb_bank_reset(adsb_bank *b, uint32_t stream);
ADSB_MUST_CHECK int adsb_bank_consumed(const adsb_bank *b, uint32_t stream, uint64_t *consumed);
ADSB_MUST_CHECK int adsb_bank_out_count(const adsb_bank *b, uint32_t stream, size_t n_in, size_t *n_out);
ADSB_MUST_CHECK int adsb_bank_inputs_for(const adsb_bank *b, uint32_t stream, size_t n_out_wanted, size_t *n_in,
                                         size_t *n_out_made);
ADSB_MUST_CHECK int adsb_bank_run_device(adsb_bank *b, int format, uint32_t n_runs, const uint32_t *streams,
                                         const void *const *device_in, const size_t *n_in, void *const *device_out_cs16,
                                         const size_t *out_cap, size_t *n_out);
ADSB_MUST_CHECK int adsb_bank_set_mixer(adsb_bank *b, const int16_t *cs_pairs, uint32_t period);
extern uint32_t adsb_bank_get_mixer(const adsb_bank *b);
ADSB_MUST_CHECK int adsb_bank_set_scale(adsb_bank *b, float scale);
extern float adsb_bank_get_scale(const adsb_bank *b);
/* Host only, for the tests: the number of descriptor blocks a bank rotates through. */
extern uint32_t adsb_bank_selftest_depth(void);

/* ---------------------------------------------------------------------------------------------------------
 * Input statistics -- opt-in per handle, off by default; with the mode off nothing observable changes: the handle makes
 * no launch and reserves no memory.  adsb_set_signal_stats counts on the 2.4 MS/s CS16 the scan reads.  Behind a
 * decimator, a resampler or a bank that is the wrong place to set a radio's gain by: a sample that hit the ADC rail at
 * 20 MS/s has been averaged with its neighbours, the DC spike and the LO leakage have been mixed and filtered away, a
 * CF32 conversion that clamps does so silently, and every output of a bank looks like band-limited noise.  This mode
 * counts where the ADC's samples still exist: on the RAW input of adsb_decim, adsb_resamp and adsb_bank, by a kernel of
 * its own (k_instat) in front of the filter's, as exact integers.
 *
 * The record.  c[m] = (re, im) is the converted CS16 sample that "Sample formats" puts in the place of x[m], BEFORE the
 * mixer: CS16 the sample itself; 8-bit T8[b], through the context's table at the time of the call; CF32 q(x) with the
 * handle's scale; REAL16 (r, 0).  A record covers a set S of input samples of one stream.  Every field is an exact
 * integer and independent of the order of addition: it equals the plain restatement with tolerance 0.
 *   adsb_input_bin(v)  0 for v == 0, else 1 + floor(log2 |v|): 0 .. 16, and -32768 lands in bin 16.  Host only.
 *   clipped            a sample with a component at a rail of the RAW format.  CS16 / REAL16: a component in {-32768,
 *                      32767}.  8-bit: a byte in {0, 255}, tested on the bytes before widening, as adsb_signal_stats
 *                      does -- the table does not enter.  CF32: a component that is not NaN and has q(x) in {-32768,
 *                      32767}.
 *   NaN                a NaN component counts its sample in n_nan, never in n_clipped; its converted value 0 enters the
 *                      sums and bin 0.
 * Samples outside the call's n_in are never counted: not the int16 behind an odd REAL16 end, not whatever the rounded-up
 * 16-byte load fetches behind the last sample, not the zero history.  The mixer, the taps and the ratio do not enter: the
 * record is the same with the mixer on, off or changed.  The sums are 64-bit and wrap beyond that: about 2^33 samples
 * between two fetches are safe (2^33 x 2^30 = 2^63 for the squares).
 *
 * Accumulation.  While the mode is on, every input sample the handle consumes is added to the handle's accumulator in
 * device memory -- in a bank, to the accumulator of the run's stream -- whichever call consumed it: *_run_device,
 * *_demod_iq piece by piece, or adsb_bank_run_device.  A call that returns ADSB_ERR_CAPACITY or ADSB_ERR_INVALID consumes
 * nothing and counts nothing; a run of no input counts nothing; *_reset leaves the accumulator alone.  "The cut is
 * invisible" extends to the record: the record of a stream is the same for any cutting into calls, with formats
 * alternating between calls.  The launch goes on the stream the filter launch uses, in front of it, in the same call.
 *
 *   adsb_instat_set_*    1: the first enable reserves the accumulator -- 208 B (208 B x N for a bank) of device memory
 *                        and as much pinned memory for the fetch -- and zeroes it, ordered on the stream like a run;
 *                        enabling a handle that is already on changes nothing.  0: later calls launch nothing, and what
 *                        was accumulated is discarded.  Never ADSB_ERR_BUSY.  ADSB_ERR_INVALID for NULL.
 *   adsb_instat_get_*    1 / 0; ADSB_ERR_INVALID for NULL
 *   adsb_instat_fetch_*  waits for everything the handle has put on the stream, writes the records that cover exactly the
 *                        inputs consumed since the previous fetch of that stream (or since the enable), and zeroes what
 *                        it fetched.  A bank fetch writes n_streams records, stream first_stream first, and touches only
 *                        that range.  ADSB_ERR_INVALID for NULL arguments, a range beyond N, or a handle whose mode is off.
 *   adsb_input_summary   folds n records into what a gain display shows -- a property, not bits: the doubles come from
 *                        libm.  A logarithm of zero comes back as -inf, never NaN, as in adsb_signal_summary.  Host
 *                        only.  ADSB_ERR_INVALID for a null `out`, or a null `s` with n > 0.
 * Recipe.  An Airspy R2 at 20 MS/s raw, its gain set by the rail hits the ADC itself saw:
 *     adsb_feed --format s16real --resample 3/25 --shift -5000000 --input-stats 1
 * and an Airspy Mini at 12 MS/s:
 *     adsb_feed --format s16real --decimate 5 --shift -3000000 --input-stats 1
 * Not here: input statistics on the scan's own entry points (adsb_set_signal_stats is that), per-call records, and
 * statistics in adsb_multi. */
#define ADSB_INPUT_BINS 17
typedef struct adsb_input_stats {
    uint64_t n_samples;              /* |S| */
    int64_t  sum_re, sum_im;         /* sum of re, of im: the DC offset times n */
    uint64_t sum_re2, sum_im2;       /* sum of re^2, of im^2: power, and the I/Q gain balance */
    int64_t  sum_re_im;              /* sum of re im: the I/Q phase error */
    uint64_t n_clipped;              /* samples with a component at a rail of the RAW format */
    uint64_t n_nan;                  /* CF32: samples with a NaN component; 0 in the other formats */
    uint64_t hist[ADSB_INPUT_BINS];  /* hist[adsb_input_bin(v)]++ for v = re and v = im (REAL16: re only) */
    uint32_t peak;                   /* max over S of max(|re|, |im|); 0 .. 32768; 0 for empty S */
    uint32_t reserved;               /* 0 */
} adsb_input_stats;                  /* 208 bytes */

/* What a gain display shows, over any number of records (adsb_input_summary). */
typedef struct adsb_input_summary_t {
    uint64_t n_records;
    uint64_t n_samples;
    double mean_power_dbfs;   /* 10 log10((sum re^2 + sum im^2) / n_samples / 32768^2) */
    double peak_dbfs;         /* 20 log10(max peak / 32768) */
    double dc_re, dc_im;      /* sum re / n_samples, sum im / n_samples, in LSB (0 when there are no samples) */
    double clipped_fraction;  /* n_clipped / n_samples (0 when there are no samples) */
    double nan_fraction;      /* n_nan / n_samples */
    double iq_gain_db;        /* 10 log10(sum re^2 / sum im^2) */
    uint32_t bits_used;       /* the highest non-empty bin (0 when there are no samples) */
    uint32_t reserved;
} adsb_input_summary_t;

ADSB_MUST_CHECK int adsb_instat_set_decim(adsb_decim *d, int enabled);
ADSB_MUST_CHECK int adsb_instat_set_resamp(adsb_resamp *r, int enabled);
ADSB_MUST_CHECK int adsb_instat_set_bank(adsb_bank *b, int enabled);
ADSB_MUST_CHECK int adsb_instat_get_decim(const adsb_decim *d);
ADSB_MUST_CHECK int adsb_instat_get_resamp(const adsb_resamp *r);
ADSB_MUST_CHECK int adsb_instat_get_bank(const adsb_bank *b);
ADSB_MUST_CHECK int adsb_instat_fetch_decim(adsb_decim *d, adsb_input_stats *out);
ADSB_MUST_CHECK int adsb_instat_fetch_resamp(adsb_resamp *r, adsb_input_stats *out);
ADSB_MUST_CHECK int adsb_instat_fetch_bank(adsb_bank *b, uint32_t first_stream, uint32_t n_streams, adsb_input_stats *out);
extern int adsb_input_bin(int16_t v);
ADSB_MUST_CHECK int adsb_input_summary(const adsb_input_stats *s, size_t n, adsb_input_summary_t *out);
/* Test hooks, host only.  _geometry: the samples of `format` a workgroup reads in one round, and the most workgroups a
 * launch gives one run (a longer run gives each workgroup several tiles); ADSB_ERR_INVALID for a format there is not.
 * _launches: how many k_instat / k_instat_bank launches the handle has made (none while the mode is off); 0 for NULL. */
ADSB_MUST_CHECK int adsb_instat_selftest_geometry(int format, uint32_t *tile_samples, uint32_t *max_groups_per_run);
extern uint64_t adsb_instat_selftest_launches_decim(const adsb_decim *d);
extern uint64_t adsb_instat_selftest_launches_resamp(const adsb_resamp *r);
extern uint64_t adsb_instat_selftest_launches_bank(const adsb_bank *b);

/* Sharded capture: one capture cut into contiguous ranges of 131072-sample buffers, one
 * range per GPU (BASELINE config 4; the reference's loop dump1090_rs/src/main.rs:161-167
 * is one stream with one process-global filter, src/icao_filter.rs:8-9).  Shards run
 * independently except for that filter, so each runs in two phases around a small host-side
 * exchange:
 *   adsb_shard_scan    scans the shard (device_iq: this shard's samples, 16-byte aligned)
 *                      and returns the 24-bit addresses its clean DF11 (IID 0) / DF17 frames
 *                      will add to the filter (src/mode_s/mod.rs:80-84, 97-99), sorted;
 *   the caller hands every shard the union of all shards' lists (a few KB);
 *   adsb_shard_finish  adds them to the shard's address superset, matches the shard's
 *                      address/parity trials against it and returns the raw trial records
 *                      (chunk = buffer index within the shard).
 * Whoever gathers all records adds each shard's first buffer index to `chunk` and replays
 * them once with adsb_replay_records: the result is the single-stream one.  Between the two
 * calls the context accepts no other work (ADSB_ERR_BUSY).  `cap` too small ->
 * ADSB_ERR_CAPACITY with the required count in *n_addrs / *n_records; for
 * adsb_shard_scan the shard stays parked and adsb_shard_finish may still be called. */
int adsb_shard_scan(adsb_ctx *ctx, const void *device_iq, size_t n_samples, uint32_t *addrs_out,
                    size_t cap, size_t *n_addrs);
int adsb_shard_finish(adsb_ctx *ctx, const uint32_t *extra_addrs, size_t n_extra,
                      adsb_trial *records_out, size_t cap, size_t *n_records);

/* ---------------------------------------------------------------------------------------------------------
 * One capture over several GPUs from ONE process (BASELINE config 4).  The reference is one process with
 * one loop and one process-global filter (dump1090_rs/src/main.rs:154-167, src/icao_filter.rs:8-9); an
 * adsb_multi keeps that shape for its caller -- one handle, one ICAO filter, one message list in the
 * reference's order -- over N devices: the capture is cut into contiguous ranges of 131072-sample buffers,
 * one per device; inside, a context and a host thread per device run the two shard phases above, the
 * learned addresses are united in memory between them, and the caller's thread replays all shards' trial
 * records once, in global (buffer, j, try_phase) order, through the one filter (a dense stream's shards are scored
 * on their devices instead -- against the filter as it stood plus what the shards before them add -- and only
 * concatenated here; a capture of >= 8192 records that the host does score --
 * a busy sky -- with the help of up to six more threads, created when the first such capture is collected: every
 * record is scored against the filter as it was plus the record numbers at which the capture's new addresses
 * enter it, which is the ordered replay's answer, computed side by side).  No process group, no
 * collective, nothing outside this library.  The result is the single-stream one, bit for bit.
 *
 *   adsb_multi_create        a context on each of devices[0..n) (a device may appear more than once: then
 *                            its shards share it), each for up to max_chunks_per_device buffers per capture
 *   adsb_multi_icao_flush    == icao_flush() for the ONE filter; applies to the captures submitted after it
 *   adsb_multi_demod_iq      a host capture of any length: cut, copied to the devices, demodulated (blocking)
 *   adsb_multi_demod_iq_device  the shards already resident: device_iq[k] / n_samples[k] = device k's range
 *                            (16-byte aligned; whole buffers except the capture's last non-empty shard;
 *                            adsb_multi_shard_range gives the even split), blocking
 *   adsb_multi_submit_iq_device / adsb_multi_collect   the same, asynchronously: up to
 *                            adsb_multi_max_in_flight (4) captures in flight, results in submission order;
 *                            the scans of capture i + 1 run while capture i is exchanged, matched and
 *                            replayed.  The samples must be complete (their producer synchronised) before
 *                            the call and unchanged until the capture is collected.
 *   adsb_multi_submit_iq     the asynchronous form for a HOST capture of at most n_devices x
 *                            max_chunks_per_device buffers: every device thread copies its range to its device in
 *                            front of its scan.  Out of memory from adsb_multi_host_alloc (pinned for every
 *                            device) the copies are DMAs, one per device over its own link, and overlap the
 *                            scans of the captures in flight; out of ordinary memory they go through the
 *                            runtime's staging buffers (a third of the rate).  The samples stay the caller's
 *                            and must not change before the capture is collected.  (Device side: a staging buffer of
 *                            max_chunks_per_device buffers per capture in flight and device, allocated the first
 *                            time the host form uses that slot and kept: up to 4 x 256 MiB per device at 512.)
 * adsb_msg.chunk is the buffer's index in the whole capture.  Errors and ADSB_ERR_CAPACITY behave as for
 * the one-device calls (adsb_multi_fetch_messages hands out the whole list of a capture whose `out` was too
 * small).  One adsb_multi is driven by one host thread at a time.  Like every entry point of this header, these leave
 * the calling thread's current HIP device as they found it.
 *
 * When a capture fails.  Every wait inside is bounded: a shard phase that has been out for 2 ms has its streams asked
 * (a stream error fails the shard), and one that is still out after the handle's timeout (adsb_multi_set_timeout_ms,
 * 30 s by default) fails it and gives the device up -- nothing more is enqueued on it, and adsb_multi_destroy leaks
 * that device's context instead of waiting for a kernel that never ends.  The capture's collect (or blocking call)
 * returns the failed shard's status, adsb_multi_last_error names the device, and the handle is POISONED: the one
 * filter and the devices' address supersets have missed that capture's additions, so the captures in flight behind it
 * and every later submission return ADSB_ERR_POISONED -- never a silently different frame list.  Collect what is in
 * flight (each returns ADSB_ERR_POISONED), then adsb_multi_icao_flush: it resets every device's context, the filter
 * and the exchange state, and the stream starts over from an empty filter, as after icao_flush().  If a device cannot
 * be reset (it was given up, or the reset itself fails) the flush returns that error and the handle stays poisoned:
 * destroy it.  adsb_multi_destroy never blocks on a device. */
typedef struct adsb_multi adsb_multi;
typedef struct {
    uint64_t n_samples;
    uint64_t n_chunks;
    uint64_t n_candidates;
    uint64_t n_ap_entries;
    uint64_t n_records;          /* trial records replayed on the host */
    uint64_t n_messages;
    uint64_t n_addrs_exchanged;  /* learned addresses handed to every device between the phases */
    uint32_t n_devices;
    uint32_t retries;            /* shards that went buffer by buffer (list overflow) */
    float ms_wall;               /* submit -> the last device's records on the host (host clock) */
    float ms_phase1_max;         /* slowest device: phase 1 issued -> its summary seen (scan + records of learned frames) */
    float ms_phase2_max;         /* slowest device: phase 2 issued -> its summary seen (set addresses, match, records) */
    float ms_phase1_span;        /* first device's phase-1 issue -> last device's phase-1 summary */
    float ms_phase2_span;        /* ... the same for phase 2: ms_wall - the two spans = what the orchestration adds */
    float ms_exchange;           /* the union of the learned addresses + handing phase 2 to every device thread */
    float ms_replay;             /* the ordered replay in adsb_multi_collect */
    float reserved;
} adsb_multi_stats;

int adsb_multi_create(adsb_multi **out, const int *devices, int n_devices, size_t max_chunks_per_device);
void adsb_multi_destroy(adsb_multi *m);
int adsb_multi_device_count(const adsb_multi *m);
int adsb_multi_max_in_flight(const adsb_multi *m);
/* Device k's contiguous share of a capture of n_samples cut n_devices ways: whole buffers, sizes that differ by at
 * most one buffer, the ragged end with whoever holds the last buffer.  Host only. */
int adsb_multi_shard_range(size_t n_samples, int n_devices, int k, size_t *first_sample, size_t *n_samples_k);
int adsb_multi_icao_flush(adsb_multi *m);
int adsb_multi_demod_iq(adsb_multi *m, const int16_t *iq_re_im, size_t n_samples, adsb_msg *out, size_t cap,
                        size_t *n_out);
int adsb_multi_demod_iq_device(adsb_multi *m, const void *const *device_iq, const size_t *n_samples, adsb_msg *out,
                               size_t cap, size_t *n_out);
int adsb_multi_submit_iq_device(adsb_multi *m, const void *const *device_iq, const size_t *n_samples);
int adsb_multi_submit_iq(adsb_multi *m, const int16_t *iq_re_im, size_t n_samples);
/* Pinned host memory every device of the adsb_multi reads by DMA (hipHostMalloc, portable).  Freed by
 * adsb_multi_host_free (ADSB_ERR_BUSY while captures are in flight) or by adsb_multi_destroy. */
int adsb_multi_host_alloc(adsb_multi *m, size_t bytes, void **out);
int adsb_multi_host_free(adsb_multi *m, void *host_ptr);
int adsb_multi_collect(adsb_multi *m, adsb_msg *out, size_t cap, size_t *n_out);
int adsb_multi_pending(const adsb_multi *m);
int adsb_multi_fetch_messages(adsb_multi *m, adsb_msg *out, size_t cap, size_t *n_out);
/* Counters and host-clock timings of the capture collected last. */
int adsb_multi_get_stats(const adsb_multi *m, adsb_multi_stats *out);
/* Table A of the one filter (4096 u32, src/icao_filter.rs:8), for inspection.  ADSB_ERR_BUSY while captures are
 * in flight. */
int adsb_multi_filter_table(const adsb_multi *m, uint32_t *out4096);
const char *adsb_multi_last_error(const adsb_multi *m);
/* How the handle's threads wait for their devices.
 *   ADSB_WAIT_SPIN   a device thread polls its shard's summary in mapped memory while anything is out on its device
 *                    (a phase's end is seen within a microsecond; costs a CPU per device while captures are in flight),
 *                    the collector spins for 2 ms before it sleeps, the replay pool's workers stay hot for 1.5 ms;
 *   ADSB_WAIT_BLOCK  the device threads sleep between looks (a timed wait on their command queue: 25 us while a
 *                    phase is young, up to 1 ms as it ages; a command wakes them at once), the collector and the pool's
 *                    workers sleep on their condition variables right away: a quarter of the CPU time, the same
 *                    throughput for a caller with several captures in flight, 4-7 % more latency for one that has a
 *                    single capture in flight (profiles/r6_wait_policy.txt).  Where the process is short of CPUs
 *                    (a cgroup quota, an affinity mask) it is the only sane form: spinning threads take the CPU from
 *                    the one that has work, or get the whole process throttled (+43-54 % per capture under 4 CPUs);
 *   ADSB_WAIT_AUTO   (default) BLOCK when the CPUs the process may use (affinity mask, cgroup cpu.max) are fewer
 *                    than 2 x (devices + 3), else SPIN; decided at create and again by this call.
 * ADSB_ERR_BUSY while captures are in flight.  adsb_multi_get_wait returns what is in effect (SPIN or BLOCK). */
#define ADSB_WAIT_AUTO 0
#define ADSB_WAIT_SPIN 1
#define ADSB_WAIT_BLOCK 2
int adsb_multi_set_wait(adsb_multi *m, int mode);
int adsb_multi_get_wait(const adsb_multi *m);
/* After this long without a shard phase finishing, the device it runs on is given up (see "When a capture fails").
 * 0 = the default, 30 000 ms.  May be called at any time. */
int adsb_multi_set_timeout_ms(adsb_multi *m, uint32_t ms);
/* The error-correction mode (adsb_set_error_correction) of every device context of the handle and of its collector's
 * replay, for the captures submitted after the call.  ADSB_ERR_INVALID for other values; ADSB_ERR_BUSY while captures
 * are in flight. */
int adsb_multi_set_error_correction(adsb_multi *m, int mode);

/* Host only, no device needed: the ordered replay every demod call ends with
 * (score_modes_message src/mode_s/mod.rs:34-139 + best-of-5 selection
 * src/demod_2400.rs:149-207 + icao_filter src/icao_filter.rs), exposed so the
 * sequential logic can be exercised on its own.  `records` may come in any order (they are
 * replayed by (chunk, j, try_phase) and left as they are).  `filter_table` is table A of the filter (4096 u32,
 * src/icao_filter.rs:8), read and updated. */
int adsb_replay_records(uint32_t *filter_table, adsb_trial *records, size_t n, adsb_msg *out,
                        size_t cap, size_t *n_out);
/* ... under an error-correction mode (ADSB_FIX_NONE: exactly adsb_replay_records; ADSB_FIX_1BIT: see
 * adsb_set_error_correction), for shard users who replay the records themselves. */
int adsb_replay_records_fix(uint32_t *filter_table, adsb_trial *records, size_t n, int mode, adsb_msg *out,
                            size_t cap, size_t *n_out);
/* The syndromes the library repairs with: syn112[b] = modes_checksum(e_b, 112) for b = 0..111 (only 5..111 are
 * repaired).  Host only, no context: for the test that pins them against the CRC of the reference. */
int adsb_selftest_fix_table(uint32_t *syn112);
/* ... and the table the scan kernels look them up in: keyed by H' = x^-56 * residual (the form in which the scan
 * holds a 112-bit trial's residual), slot = (H' * *mult) >> 23 of 512 (`cap` >= 512), entry = H' | b << 24, 0 empty.
 * Host only, no context: for the test that it is collision-free and complete. */
int adsb_selftest_fix_hash(uint32_t *mult, uint32_t *table, size_t cap);
/* ... and the pair table of ADSB_FIX_2BIT, which the scan kernels look up in global memory: keyed by
 * H'(a) ^ H'(b) = x^(55-a) + x^(55-b), 2^params4[2] buckets of two entries {key | a << 24, (syn(a) ^ syn(b)) | b << 24}
 * (4 u32 a bucket, {0, 0} empty); a key sits in bucket (key * params4[i]) >> (32 - params4[2]) for i = 0 or 1, so a
 * lookup reads params4[3] = 4 entries at most.  `buckets` gets 4 << params4[2] u32 (`cap` >= 32768).  Host only, no
 * context: for the test that it is complete and that no key sits outside its buckets. */
int adsb_selftest_fix2_table(uint32_t *params4, uint32_t *buckets, size_t cap);

/* Device self-test: the repair the scoring kernels find for each of `n` CRC residuals (24 bits) under `mode` (ADSB_FIX_NONE,
 * ADSB_FIX_1BIT, ADSB_FIX_2BIT) -- the very device function k_score and k_emit repair with, over the context's tables.
 * out[i] = a | b << 8: 0xFF | b << 8 when residuals[i] == syn(b), b in 5..111 (modes 1 and 3); a | b << 8 when it is
 * syn(a) ^ syn(b), 5 <= a < b <= 111 (mode 3 only); 0xFFFF ("none") for everything else, zero included.  Lets a test sweep
 * all 107 + 5671 syndromes and any number of non-syndromes without building IQ for each.  ADSB_ERR_BUSY while passes are
 * pending; n <= 2^24. */
int adsb_selftest_fix_lookup(adsb_ctx *ctx, const uint32_t *residuals, size_t n, int mode, uint32_t *out);

/* Device self-test: digest of the magnitude tail (sqrt, *65535+0.5, saturating
 * cast; src/utils.rs:54-55) over `count` consecutive f32 bit patterns of
 * X = im^2 + rn(re^2) starting at `first_bits`.  sum = sum of the u16 outputs,
 * xor = XOR of (out+1)*(2*bits+1).  A test sweeps all X in [0, 2^31] with it. */
int adsb_selftest_mag_digest(adsb_ctx *ctx, uint32_t first_bits, uint32_t count,
                             uint64_t *sum_out, uint64_t *xor_out);

/* Device self-test: the intermediate lists of one blocking pass over device-resident IQ, so that a
 * test can compare stages, not only frames, with the CPU restatement of the reference:
 *   cand[]  every position the gates let through (check_preamble + 3.5 dB + quiet samples,
 *           src/demod_2400.rs:127-146), as buffer << 32 | j, ascending;
 *   ap[]    every address/parity trial (DF 0,4,5,16,20,21,24-31, src/mode_s/mod.rs:56-72,110-135) with
 *           its CRC residual (src/crc.rs:263-282), as buffer << 45 | j << 28 | try_phase << 24 | residual,
 *           ascending.
 * The context's filter is not touched.  ADSB_ERR_CAPACITY with the required counts when a list does
 * not fit; ADSB_ERR_BUSY while passes are pending. */
int adsb_selftest_stage_lists(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples, uint64_t *cand,
                              size_t cand_cap, size_t *n_cand, uint64_t *ap, size_t ap_cap, size_t *n_ap);

/* Device self-test, the two stages in front of cand[]: every position at which check_preamble returns
 * Some (src/demod_2400.rs:215-321) -> preamble[], and those that also pass the 3.5 dB test (:129) ->
 * snr[]; both as buffer << 32 | j, ascending (cand[] above is the subset of snr[] that also passes the
 * quiet samples, :135-146).  The kernel writes them from the reference's own sequence of tests applied
 * to its bit-parallel pattern matches, next to the verdict of its production gates; the call fails with
 * ADSB_ERR_HIP if the two ever disagree.  Same conventions as adsb_selftest_stage_lists. */
int adsb_selftest_gate_stages(adsb_ctx *ctx, const void *device_iq_re_im, size_t n_samples, uint64_t *preamble,
                              size_t preamble_cap, size_t *n_preamble, uint64_t *snr, size_t snr_cap, size_t *n_snr);

/* Test hook for the one-launch pass (passes of at most 16 buffers): inside such a pass a workgroup matches
 * its address/parity trials once every tile before its own has published its address bits, and waits for
 * that at most `polls` polls (200 by default, ~0.2 ms); a workgroup that gives up leaves the decision to a
 * second look by the pass's last workgroup.  0 makes every workgroup give up at once, so that a test can
 * run the second look on purpose; results never depend on the value.  ADSB_ERR_BUSY while passes are pending. */
int adsb_selftest_set_order_polls(adsb_ctx *ctx, uint32_t polls);

/* Test hooks for adsb_multi (0 = the default; results never depend on any of them; ADSB_ERR_BUSY while captures are in flight):
 * fresh_cap     a shard's scan lists the addresses its trials can add to the filter, at most this many (16384); a
 *               capture with more aircraft falls back to reading them out of its trial records -- a small value lets a
 *               test take that fallback on purpose;
 * parallel_min  captures of at least this many trial records (8192) are scored by several host threads at once;
 * score_mode    0: a dense stream's shards (contexts of more than 16 buffers) are scored on their devices; 1: never;
 *               2: scored, but the collector refuses the result and fetches the records instead (the path a filter
 *               table about to fill up takes). */
int adsb_multi_selftest_tune(adsb_multi *m, uint32_t fresh_cap, uint32_t parallel_min, uint32_t score_mode);
/* Fault injection for the tests of "When a capture fails": shard `shard` of the capture submitted `captures_from_now`
 * submissions after this call (0 = the next one) fails in the given way; kind 0 disarms.
 *   ADSB_FAULT_PHASE1   its first phase is refused as if the launch had failed (ADSB_ERR_HIP);
 *   ADSB_FAULT_PHASE2   ... its second phase;
 *   ADSB_FAULT_HANG     its first phase is treated as never finishing: the timeout path, the device is given up;
 *   ADSB_FAULT_RECORDS  its records are refused when the second phase has landed, as if their checksum had failed. */
#define ADSB_FAULT_PHASE1 1
#define ADSB_FAULT_PHASE2 2
#define ADSB_FAULT_HANG 3
#define ADSB_FAULT_RECORDS 4
int adsb_multi_selftest_fail(adsb_multi *m, uint32_t captures_from_now, int shard, int kind);
/* ... and what the shards did so far: out8[0] shards whose records the host had to put in order, [1] shards that took
 * the fresh_cap fallback, [2] shards whose second phase ordered its records on the device (a dense stream's), [3] captures
 * whose records were scored by several host threads at once, [4] shards scored on their device, [5] such results the
 * collector used, [6] ... and refused; [7] 1 while the handle is poisoned. */
int adsb_multi_selftest_counters(const adsb_multi *m, uint64_t *out8);

/* Host only, no context: the ordered replay done by several threads at once, as adsb_multi_collect does it for captures
 * of tens of thousands of records (csrc/adsb_replay_host.h: ParallelReplay) -- the records are put in order, cut into
 * `runs` runs at buffer boundaries (the shards), planned into `parts` parts and scanned / scored by `threads` threads.
 * Same arguments and results as adsb_replay_records; *went_parallel = 0 when the plan was refused (too few records, a
 * filter table that could fill up) and the records were replayed serially.  For the tests that pin it to the serial
 * replay and to the oracle. */
int adsb_selftest_parallel_replay(uint32_t *filter_table, const adsb_trial *records, size_t n, int runs, int parts, int threads,
                                  adsb_msg *out, size_t cap, size_t *n_out, int *went_parallel);
/* ... under an error-correction mode (adsb_set_error_correction; ADSB_FIX_NONE is the call above). */
int adsb_selftest_parallel_replay_fix(uint32_t *filter_table, const adsb_trial *records, size_t n, int runs, int parts,
                                      int threads, int mode, adsb_msg *out, size_t cap, size_t *n_out, int *went_parallel);

/* The 256-entry CRC-24 table the host replay scores with (src/crc.rs:3-260 CRC_TABLE): for the test that
 * pins it against the reference's constants.  Host only, no context. */
int adsb_selftest_crc_table(uint32_t *out256);

/* Host only, no context: the address exchange of a sharded capture as the library does it -- the 24-bit
 * addresses the replay of `records` can add to the filter (clean DF11 with IID 0, DF17: src/mode_s/mod.rs:80-84,
 * 97-99), sorted, without duplicates and without those in `known` (any order).  For the tests that run the
 * host-only code under sanitizers. */
int adsb_selftest_learned_union(const adsb_trial *records, size_t n, const uint32_t *known, size_t n_known,
                                uint32_t *out, size_t cap, size_t *n_out);

int adsb_get_stats(const adsb_ctx *ctx, adsb_stats *out);
/* Diagnostic: how many collected passes handed the host their trial records out of
 * (buffer, j, try_phase) order, so that the host replay had to sort them first.  Passes of more
 * than 16 buffers are put in order on the device; small passes and the overflow fallback are not. */
uint64_t adsb_host_sorts(const adsb_ctx *ctx);
/* Diagnostic: how many collected passes the host scored itself (the ordered replay of
 * score_modes_message / best-of-5, src/mode_s/mod.rs:34-139, src/demod_2400.rs:184-207) instead of
 * taking the messages the device scored.  Passes of more than 16 buffers in a steady pipeline are
 * scored on the device against a device-resident copy of the ICAO filter -- in every error-correction mode: the
 * device repairs the DF17/18 trials of an ADSB_FIX_1BIT / ADSB_FIX_2BIT pass itself --; small passes, fallbacks,
 * a filter close to its 4096 entries and the passes in flight behind any of those are not. */
uint64_t adsb_host_replays(const adsb_ctx *ctx);
/* Diagnostic: how many passes of a few buffers were run a second time.  Such a pass is a single launch
 * that does not wait for the passes still in flight beside it; when one of those turns out to have added
 * a NEW address to the filter (src/icao_filter.rs:46-62) -- rare once a receiver has seen the aircraft
 * around it -- the later pass's address/parity trials may have been matched too early, and it is redone
 * behind everything else so that the result stays the reference's. */
uint64_t adsb_host_rematches(const adsb_ctx *ctx);
const char *adsb_strerror(int status);
/* Text of the last HIP failure on this context ("" if none). */
const char *adsb_last_error(const adsb_ctx *ctx);
/* Library / kernel generation string, e.g. "adsb_hip 0.1 gfx950". */
const char *adsb_version(void);

#ifdef __cplusplus
}
#endif
#endif
