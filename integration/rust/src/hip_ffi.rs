//! `extern "C"` declarations for `include/adsb_hip.h` (libadsb_hip.so, gfx950).
//! NOT COMPILED in the build image (no Rust toolchain there).  It cannot drift from the header
//! unnoticed: tests/test_rust_shim.py parses this file and include/adsb_hip.h and compares every
//! function (name, arity, argument and return types), the status constants and the field order,
//! types, offsets and sizes of the three structs (which tests/abi_host.c also pins with
//! _Static_assert from the C side).
#![allow(dead_code)]
use std::os::raw::{c_char, c_int, c_void};

pub const ADSB_OK: c_int = 0;
pub const ADSB_ERR_INVALID: c_int = -1;
pub const ADSB_ERR_NO_DEVICE: c_int = -2;
pub const ADSB_ERR_HIP: c_int = -3;
pub const ADSB_ERR_TOO_LONG: c_int = -4;
pub const ADSB_ERR_CAPACITY: c_int = -5;
pub const ADSB_ERR_NOMEM: c_int = -6;
pub const ADSB_ERR_BUSY: c_int = -7;
pub const ADSB_ERR_POISONED: c_int = -8;

// error-correction modes (adsb_set_error_correction) and the score of a repaired message
pub const ADSB_FIX_NONE: i32 = 0;
pub const ADSB_FIX_1BIT: i32 = 1;
pub const ADSB_SCORE_FIXED_1BIT: i32 = 1200;
pub const ADSB_FIX_2BIT: i32 = 3;
pub const ADSB_SCORE_FIXED_2BIT: i32 = 1100;

/// `adsb_msg`: `ModeSMessage` (src/demod_2400.rs:92-102) + provenance.  40 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct AdsbMsg {
    pub msg: [u8; 14],
    pub len: u8, // 7 | 14 == buffer().len()
    pub try_phase: u8,
    pub score: i32,
    pub j: u32,
    pub chunk: u64,
    pub signal_level: f64,
}

/// `adsb_trial`: one raw trial message, before scoring.  32 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct AdsbTrial {
    pub power: u64,
    pub chunk: u32,
    pub j_tp: u32, // j | try_phase << 24
    pub msg: [u8; 14],
    pub pad: u16,
}

/// `adsb_stats`: counters and timings of the most recent call.  72 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct AdsbStats {
    pub n_samples: u64,
    pub n_chunks: u64,
    pub n_candidates: u64,
    pub n_ap_entries: u64,
    pub n_records: u64,
    pub n_messages: u64,
    pub ms_scan: f32,
    pub ms_match: f32,
    pub ms_records: f32,
    pub ms_total_device: f32,
    pub retries: u32,
    pub ms_scan_exclusive: f32,
}

/// `adsb_multi_stats`: counters and host-clock timings of the capture an `adsb_multi` collected last.  96 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct AdsbMultiStats {
    pub n_samples: u64,
    pub n_chunks: u64,
    pub n_candidates: u64,
    pub n_ap_entries: u64,
    pub n_records: u64,
    pub n_messages: u64,
    pub n_addrs_exchanged: u64,
    pub n_devices: u32,
    pub retries: u32,
    pub ms_wall: f32,
    pub ms_phase1_max: f32,
    pub ms_phase2_max: f32,
    pub ms_phase1_span: f32,
    pub ms_phase2_span: f32,
    pub ms_exchange: f32,
    pub ms_replay: f32,
    pub reserved: f32,
}

/// `adsb_signal_stats`: one 131072-sample buffer's signal record (opt-in, `adsb_set_signal_stats`).  272 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct AdsbSignalStats {
    pub chunk: u64,
    pub sum_power: u64,
    pub n_samples: u32,
    pub peak: u32,
    pub n_strong: u32,
    pub n_clipped: u32,
    pub hist: [u32; 60],
}

/// `adsb_signal_summary_t`: what `adsb_signal_summary` makes of any number of records.  56 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct AdsbSignalSummary {
    pub n_buffers: u64,
    pub n_samples: u64,
    pub mean_power_dbfs: f64,
    pub peak_dbfs: f64,
    pub median_dbfs: f64,
    pub clipped_fraction: f64,
    pub strong_fraction: f64,
}

pub const ADSB_INPUT_BINS: usize = 17;

/// `adsb_input_stats`: the integer record of a set of raw input samples of a decimator, a resampler or one stream of a
/// bank (opt-in, `adsb_instat_set_*`).  208 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct AdsbInputStats {
    pub n_samples: u64,
    pub sum_re: i64,
    pub sum_im: i64,
    pub sum_re2: u64,
    pub sum_im2: u64,
    pub sum_re_im: i64,
    pub n_clipped: u64,
    pub n_nan: u64,
    pub hist: [u64; 17],
    pub peak: u32,
    pub reserved: u32,
}

/// `adsb_input_summary_t`: what `adsb_input_summary` makes of any number of records.  80 bytes.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct AdsbInputSummary {
    pub n_records: u64,
    pub n_samples: u64,
    pub mean_power_dbfs: f64,
    pub peak_dbfs: f64,
    pub dc_re: f64,
    pub dc_im: f64,
    pub clipped_fraction: f64,
    pub nan_fraction: f64,
    pub iq_gain_db: f64,
    pub bits_used: u32,
    pub reserved: u32,
}

#[repr(C)]
pub struct AdsbCtx {
    _private: [u8; 0],
}

/// An integer FIR decimator in front of the scan, for IQ sampled at a multiple of 2.4 MS/s (`adsb_decim_*`).
#[repr(C)]
pub struct AdsbDecim {
    _private: [u8; 0],
}

pub const ADSB_DECIM_CS16: i32 = 0;
pub const ADSB_DECIM_8BIT: i32 = 1;
pub const ADSB_DECIM_CF32: i32 = 2;
pub const ADSB_DECIM_REAL16: i32 = 3;

/// An exact-integer L/M resampler in front of the scan, for IQ at 2.5, 3, 6, 8, 10, 20 MS/s and the like (`adsb_resamp_*`).
#[repr(C)]
pub struct AdsbResamp {
    _private: [u8; 0],
}

pub const ADSB_RESAMP_CS16: i32 = ADSB_DECIM_CS16;
pub const ADSB_RESAMP_8BIT: i32 = ADSB_DECIM_8BIT;
pub const ADSB_RESAMP_CF32: i32 = ADSB_DECIM_CF32;
pub const ADSB_RESAMP_REAL16: i32 = ADSB_DECIM_REAL16;

/// Many resampler streams of one ratio and one filter, advanced by one launch (`adsb_bank_*`).
#[repr(C)]
pub struct AdsbBank {
    _private: [u8; 0],
}

pub const ADSB_BANK_ALL: u32 = 0xFFFF_FFFF;

/// One capture over several GPUs from one process: one handle, one filter (`adsb_multi_*`).
#[repr(C)]
pub struct AdsbMulti {
    _private: [u8; 0],
}

// (edition 2024, Cargo.toml:7: extern blocks are `unsafe extern`)
#[link(name = "adsb_hip")]
unsafe extern "C" {
    pub fn adsb_create(out: *mut *mut AdsbCtx, device: c_int, max_chunks: usize) -> c_int;
    pub fn adsb_destroy(ctx: *mut AdsbCtx);
    pub fn adsb_set_stream(ctx: *mut AdsbCtx, hip_stream: *mut c_void) -> c_int;
    pub fn adsb_set_profiling(ctx: *mut AdsbCtx, level: c_int) -> c_int;
    pub fn adsb_set_carry_over(ctx: *mut AdsbCtx, enabled: c_int) -> c_int; // opt-in, not the reference's semantics
    pub fn adsb_set_error_correction(ctx: *mut AdsbCtx, mode: c_int) -> c_int; // opt-in: ADSB_FIX_1BIT, ADSB_FIX_2BIT
    pub fn adsb_get_error_correction(ctx: *const AdsbCtx) -> c_int;
    pub fn adsb_set_signal_stats(ctx: *mut AdsbCtx, enabled: c_int) -> c_int; // opt-in: one AdsbSignalStats per buffer
    pub fn adsb_get_signal_stats(ctx: *const AdsbCtx) -> c_int;
    pub fn adsb_signal_bin(m: u16) -> c_int;
    pub fn adsb_selftest_signal_launches(ctx: *const AdsbCtx) -> u64;
    pub fn adsb_icao_flush(ctx: *mut AdsbCtx) -> c_int;
    pub fn adsb_to_mag(ctx: *mut AdsbCtx, iq_re_im: *const i16, n: usize, data_out: *mut u16, length_out: *mut usize) -> c_int;
    pub fn adsb_demodulate2400(ctx: *mut AdsbCtx, data: *const u16, length: usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_demod_iq(ctx: *mut AdsbCtx, iq_re_im: *const i16, n_samples: usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_demod_iq_device(ctx: *mut AdsbCtx, device_iq: *const c_void, n_samples: usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_submit_iq_device(ctx: *mut AdsbCtx, device_iq: *const c_void, n_samples: usize) -> c_int;
    pub fn adsb_collect(ctx: *mut AdsbCtx, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_pending(ctx: *const AdsbCtx) -> c_int;
    pub fn adsb_max_in_flight(ctx: *const AdsbCtx) -> c_int;
    pub fn adsb_fetch_messages(ctx: *mut AdsbCtx, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_ring_create(ctx: *mut AdsbCtx, samples_per_slot: usize) -> c_int;
    pub fn adsb_ring_acquire(ctx: *mut AdsbCtx, host_iq_re_im: *mut *mut i16, capacity_samples: *mut usize) -> c_int;
    pub fn adsb_ring_submit(ctx: *mut AdsbCtx, n_samples: usize) -> c_int;
    pub fn adsb_ring_create_u8(ctx: *mut AdsbCtx, samples_per_slot: usize) -> c_int;
    pub fn adsb_ring_acquire_u8(ctx: *mut AdsbCtx, host_iq_re_im: *mut *mut u8, capacity_samples: *mut usize) -> c_int;
    pub fn adsb_set_u8_table(ctx: *mut AdsbCtx, table256: *const i16) -> c_int;
    pub fn adsb_to_mag_u8(ctx: *mut AdsbCtx, iq_re_im: *const u8, n: usize, data_out: *mut u16, length_out: *mut usize) -> c_int;
    pub fn adsb_demod_iq_u8(ctx: *mut AdsbCtx, iq_re_im: *const u8, n_samples: usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_demod_iq_device_u8(ctx: *mut AdsbCtx, device_iq_re_im: *const c_void, n_samples: usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_submit_iq_device_u8(ctx: *mut AdsbCtx, device_iq_re_im: *const c_void, n_samples: usize) -> c_int;
    pub fn adsb_selftest_u8_table(ctx: *mut AdsbCtx, out256: *mut i16) -> c_int;
    // many receivers, one pass: one filter per receiver, the receiver of every buffer named by a map
    pub fn adsb_set_receivers(ctx: *mut AdsbCtx, n_receivers: u32) -> c_int;
    pub fn adsb_get_receivers(ctx: *const AdsbCtx) -> c_int;
    pub fn adsb_icao_flush_receiver(ctx: *mut AdsbCtx, receiver: u32) -> c_int;
    pub fn adsb_receiver_filter_table(ctx: *const AdsbCtx, receiver: u32, out4096: *mut u32) -> c_int;
    pub fn adsb_demod_iq_rx(ctx: *mut AdsbCtx, iq_re_im: *const i16, n_samples: usize, receiver_of_buffer: *const u32, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_demod_iq_device_rx(ctx: *mut AdsbCtx, device_iq_re_im: *const c_void, n_samples: usize, receiver_of_buffer: *const u32, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_submit_iq_device_rx(ctx: *mut AdsbCtx, device_iq_re_im: *const c_void, n_samples: usize, receiver_of_buffer: *const u32) -> c_int;
    pub fn adsb_demod_iq_rx_u8(ctx: *mut AdsbCtx, iq_re_im: *const u8, n_samples: usize, receiver_of_buffer: *const u32, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_demod_iq_device_rx_u8(ctx: *mut AdsbCtx, device_iq_re_im: *const c_void, n_samples: usize, receiver_of_buffer: *const u32, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_submit_iq_device_rx_u8(ctx: *mut AdsbCtx, device_iq_re_im: *const c_void, n_samples: usize, receiver_of_buffer: *const u32) -> c_int;
    pub fn adsb_ring_submit_rx(ctx: *mut AdsbCtx, n_samples: usize, receiver_of_buffer: *const u32) -> c_int;
    pub fn adsb_replay_records_rx(filter_tables: *mut u32, n_receivers: u32, receiver_of_buffer: *const u32, n_buffers: usize, records: *mut AdsbTrial, n: usize, mode: c_int, threads: c_int, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_selftest_rx_tune(ctx: *mut AdsbCtx, parallel_min: u32) -> c_int;
    pub fn adsb_selftest_rx_counters(ctx: *const AdsbCtx, out4: *mut u64) -> c_int;
    // ... scored on the device, per receiver (opt-in), and its test hooks
    pub fn adsb_set_receiver_scoring(ctx: *mut AdsbCtx, enabled: c_int) -> c_int;
    pub fn adsb_get_receiver_scoring(ctx: *const AdsbCtx) -> c_int;
    pub fn adsb_selftest_rx_score_counters(ctx: *const AdsbCtx, out4: *mut u64) -> c_int;
    pub fn adsb_selftest_rx_score_tune(ctx: *mut AdsbCtx, set_lg: u32, probe_max: u32) -> c_int;
    pub fn adsb_selftest_rx_set_lookup(ctx: *mut AdsbCtx, keys: *const u64, n_keys: usize, queries: *const u64, n_q: usize, out: *mut u32) -> c_int;
    pub fn adsb_rx_set_home(key: u64, set_lg: u32) -> u32;
    pub fn adsb_set_receiver_carry(ctx: *mut AdsbCtx, enabled: c_int) -> c_int;
    pub fn adsb_get_receiver_carry(ctx: *const AdsbCtx) -> c_int;
    pub fn adsb_receiver_carry_reset(ctx: *mut AdsbCtx, receiver: u32) -> c_int;
    pub fn adsb_selftest_rx_seam_tune(ctx: *mut AdsbCtx, list_cap: u32) -> c_int;
    pub fn adsb_selftest_rx_seam_counters(ctx: *const AdsbCtx, out4: *mut u64) -> c_int;
    // ... receiver seams AND scoring on the device, as one mode (opt-in), and its test hooks
    pub fn adsb_set_receiver_carry_scoring(ctx: *mut AdsbCtx, enabled: c_int) -> c_int;
    pub fn adsb_get_receiver_carry_scoring(ctx: *const AdsbCtx) -> c_int;
    pub fn adsb_selftest_rx_seam_score_counters(ctx: *const AdsbCtx, out4: *mut u64) -> c_int;
    pub fn adsb_selftest_reservations(ctx: *const AdsbCtx) -> u64;
    pub fn adsb_shard_scan(ctx: *mut AdsbCtx, device_iq: *const c_void, n_samples: usize, addrs_out: *mut u32, cap: usize, n_addrs: *mut usize) -> c_int;
    pub fn adsb_shard_finish(ctx: *mut AdsbCtx, extra_addrs: *const u32, n_extra: usize, records_out: *mut AdsbTrial, cap: usize, n_records: *mut usize) -> c_int;
    pub fn adsb_multi_create(out: *mut *mut AdsbMulti, devices: *const c_int, n_devices: c_int, max_chunks_per_device: usize) -> c_int;
    pub fn adsb_multi_destroy(m: *mut AdsbMulti);
    pub fn adsb_multi_device_count(m: *const AdsbMulti) -> c_int;
    pub fn adsb_multi_max_in_flight(m: *const AdsbMulti) -> c_int;
    pub fn adsb_multi_shard_range(n_samples: usize, n_devices: c_int, k: c_int, first_sample: *mut usize, n_samples_k: *mut usize) -> c_int;
    pub fn adsb_multi_icao_flush(m: *mut AdsbMulti) -> c_int;
    pub fn adsb_multi_demod_iq(m: *mut AdsbMulti, iq_re_im: *const i16, n_samples: usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_multi_demod_iq_device(m: *mut AdsbMulti, device_iq: *const *const c_void, n_samples: *const usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_multi_submit_iq_device(m: *mut AdsbMulti, device_iq: *const *const c_void, n_samples: *const usize) -> c_int;
    pub fn adsb_multi_submit_iq(m: *mut AdsbMulti, iq_re_im: *const i16, n_samples: usize) -> c_int;
    pub fn adsb_multi_host_alloc(m: *mut AdsbMulti, bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn adsb_multi_host_free(m: *mut AdsbMulti, host_ptr: *mut c_void) -> c_int;
    pub fn adsb_multi_collect(m: *mut AdsbMulti, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_multi_pending(m: *const AdsbMulti) -> c_int;
    pub fn adsb_multi_fetch_messages(m: *mut AdsbMulti, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_multi_get_stats(m: *const AdsbMulti, out: *mut AdsbMultiStats) -> c_int;
    pub fn adsb_multi_filter_table(m: *const AdsbMulti, out4096: *mut u32) -> c_int;
    pub fn adsb_multi_last_error(m: *const AdsbMulti) -> *const c_char;
    pub fn adsb_multi_set_wait(m: *mut AdsbMulti, mode: c_int) -> c_int;
    pub fn adsb_multi_get_wait(m: *const AdsbMulti) -> c_int;
    pub fn adsb_multi_set_timeout_ms(m: *mut AdsbMulti, ms: u32) -> c_int;
    pub fn adsb_multi_set_error_correction(m: *mut AdsbMulti, mode: c_int) -> c_int;
    pub fn adsb_replay_records(filter_table: *mut u32, records: *mut AdsbTrial, n: usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_replay_records_fix(filter_table: *mut u32, records: *mut AdsbTrial, n: usize, mode: c_int, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_selftest_fix_table(syn112: *mut u32) -> c_int;
    pub fn adsb_selftest_fix_hash(mult: *mut u32, table: *mut u32, cap: usize) -> c_int;
    pub fn adsb_selftest_fix2_table(params4: *mut u32, buckets: *mut u32, cap: usize) -> c_int;
    pub fn adsb_format_raw(msg: *const AdsbMsg, out: *mut c_char, out_size: usize) -> c_int;
    pub fn adsb_read_test_data(path: *const c_char, iq_re_im: *mut i16, max_samples: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_selftest_fix_lookup(ctx: *mut AdsbCtx, residuals: *const u32, n: usize, mode: c_int, out: *mut u32) -> c_int;
    pub fn adsb_selftest_mag_digest(ctx: *mut AdsbCtx, first_bits: u32, count: u32, sum_out: *mut u64, xor_out: *mut u64) -> c_int;
    pub fn adsb_selftest_stage_lists(ctx: *mut AdsbCtx, device_iq_re_im: *const c_void, n_samples: usize, cand: *mut u64, cand_cap: usize, n_cand: *mut usize, ap: *mut u64, ap_cap: usize, n_ap: *mut usize) -> c_int;
    pub fn adsb_selftest_gate_stages(ctx: *mut AdsbCtx, device_iq_re_im: *const c_void, n_samples: usize, preamble: *mut u64, preamble_cap: usize, n_preamble: *mut usize, snr: *mut u64, snr_cap: usize, n_snr: *mut usize) -> c_int;
    pub fn adsb_selftest_set_order_polls(ctx: *mut AdsbCtx, polls: u32) -> c_int;
    pub fn adsb_multi_selftest_tune(m: *mut AdsbMulti, fresh_cap: u32, parallel_min: u32, score_mode: u32) -> c_int;
    pub fn adsb_multi_selftest_fail(m: *mut AdsbMulti, captures_from_now: u32, shard: c_int, kind: c_int) -> c_int;
    pub fn adsb_multi_selftest_counters(m: *const AdsbMulti, out8: *mut u64) -> c_int;
    pub fn adsb_selftest_parallel_replay(filter_table: *mut u32, records: *const AdsbTrial, n: usize, runs: c_int, parts: c_int, threads: c_int, out: *mut AdsbMsg, cap: usize, n_out: *mut usize, went_parallel: *mut c_int) -> c_int;
    pub fn adsb_selftest_parallel_replay_fix(filter_table: *mut u32, records: *const AdsbTrial, n: usize, runs: c_int, parts: c_int, threads: c_int, mode: c_int, out: *mut AdsbMsg, cap: usize, n_out: *mut usize, went_parallel: *mut c_int) -> c_int;
    pub fn adsb_selftest_crc_table(out256: *mut u32) -> c_int;
    pub fn adsb_selftest_learned_union(records: *const AdsbTrial, n: usize, known: *const u32, n_known: usize, out: *mut u32, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_get_stats(ctx: *const AdsbCtx, out: *mut AdsbStats) -> c_int;
    pub fn adsb_host_sorts(ctx: *const AdsbCtx) -> u64;
    pub fn adsb_host_replays(ctx: *const AdsbCtx) -> u64;
    pub fn adsb_host_register(ctx: *mut AdsbCtx, host_ptr: *mut c_void, bytes: usize) -> c_int;
    pub fn adsb_host_unregister(ctx: *mut AdsbCtx, host_ptr: *mut c_void) -> c_int;
    pub fn adsb_host_rematches(ctx: *const AdsbCtx) -> u64;
    pub fn adsb_strerror(status: c_int) -> *const c_char;
    pub fn adsb_last_error(ctx: *const AdsbCtx) -> *const c_char;
    pub fn adsb_version() -> *const c_char;
    pub fn adsb_decim_selftest_tile() -> u32;
    pub fn adsb_resamp_selftest_tile(up: u32, down: u32) -> u32;
}

// The two calls that take the signal records by pointer (the header marks them ADSB_MUST_CHECK); compared with the
// header by tests/test_signal_stats_cpu.py.
#[link(name = "adsb_hip")]
unsafe extern "C" {
    pub fn adsb_fetch_signal_stats(ctx: *mut AdsbCtx, out: *mut AdsbSignalStats, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_signal_summary(s: *const AdsbSignalStats, n: usize, out: *mut AdsbSignalSummary) -> c_int;
}

// The decimator's calls, which take its handle (the header marks them ADSB_MUST_CHECK, the destructor `extern`); compared
// with the header by tests/test_decim_cpu.py.
#[link(name = "adsb_hip")]
unsafe extern "C" {
    pub fn adsb_decim_create(ctx: *mut AdsbCtx, factor: u32, taps: *const i16, n_taps: u32, shift: u32, out: *mut *mut AdsbDecim) -> c_int;
    pub fn adsb_decim_destroy(d: *mut AdsbDecim);
    pub fn adsb_decim_reset(d: *mut AdsbDecim) -> c_int;
    pub fn adsb_decim_out_count(d: *const AdsbDecim, n_in: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_decim_run_device(d: *mut AdsbDecim, format: c_int, device_in: *const c_void, n_in: usize, device_out_cs16: *mut c_void, out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_decim_demod_iq(d: *mut AdsbDecim, format: c_int, host_iq: *const c_void, n_in: usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_decim_default_taps(factor: u32, taps: *mut i16, cap: usize, n_taps: *mut u32, shift: *mut u32) -> c_int;
}

// The resampler's calls (the header marks them ADSB_MUST_CHECK, the destructor `extern`); compared with the header by
// tests/test_resamp_cpu.py.
#[link(name = "adsb_hip")]
unsafe extern "C" {
    pub fn adsb_resamp_create(ctx: *mut AdsbCtx, up: u32, down: u32, taps: *const i16, n_taps: u32, shift: u32, out: *mut *mut AdsbResamp) -> c_int;
    pub fn adsb_resamp_destroy(r: *mut AdsbResamp);
    pub fn adsb_resamp_reset(r: *mut AdsbResamp) -> c_int;
    pub fn adsb_resamp_out_count(r: *const AdsbResamp, n_in: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_resamp_run_device(r: *mut AdsbResamp, format: c_int, device_in: *const c_void, n_in: usize, device_out_cs16: *mut c_void, out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_resamp_demod_iq(r: *mut AdsbResamp, format: c_int, host_iq: *const c_void, n_in: usize, out: *mut AdsbMsg, cap: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_resamp_default_taps(up: u32, down: u32, taps: *mut i16, cap: usize, n_taps: *mut u32, shift: *mut u32) -> c_int;
    pub fn adsb_resamp_ratio_for_rate(rate_hz: u32, up: *mut u32, down: *mut u32) -> c_int;
    pub fn adsb_resamp_plan(up: u32, down: u32, consumed: u64, n_in: u64, first_n: *mut u64, n_out: *mut u64) -> c_int;
}

// A bank of resampler streams advanced by one launch (include/adsb_hip.h, "Resampler banks"; the header marks the calls
// ADSB_MUST_CHECK or `extern`); compared with the header by tests/test_bank_cpu.py.
#[link(name = "adsb_hip")]
unsafe extern "C" {
    pub fn adsb_bank_create(ctx: *mut AdsbCtx, n_streams: u32, up: u32, down: u32, taps: *const i16, n_taps: u32, shift: u32, out: *mut *mut AdsbBank) -> c_int;
    pub fn adsb_bank_destroy(b: *mut AdsbBank);
    pub fn adsb_bank_streams(b: *const AdsbBank) -> u32;
    pub fn adsb_bank_reset(b: *mut AdsbBank, stream: u32) -> c_int;
    pub fn adsb_bank_consumed(b: *const AdsbBank, stream: u32, consumed: *mut u64) -> c_int;
    pub fn adsb_bank_out_count(b: *const AdsbBank, stream: u32, n_in: usize, n_out: *mut usize) -> c_int;
    pub fn adsb_bank_inputs_for(b: *const AdsbBank, stream: u32, n_out_wanted: usize, n_in: *mut usize, n_out_made: *mut usize) -> c_int;
    pub fn adsb_bank_run_device(b: *mut AdsbBank, format: c_int, n_runs: u32, streams: *const u32, device_in: *const *const c_void, n_in: *const usize, device_out_cs16: *const *mut c_void, out_cap: *const usize, n_out: *mut usize) -> c_int;
    pub fn adsb_bank_set_mixer(b: *mut AdsbBank, cs_pairs: *const i16, period: u32) -> c_int;
    pub fn adsb_bank_get_mixer(b: *const AdsbBank) -> u32;
    pub fn adsb_bank_set_scale(b: *mut AdsbBank, scale: f32) -> c_int;
    pub fn adsb_bank_get_scale(b: *const AdsbBank) -> f32;
    pub fn adsb_bank_selftest_depth() -> u32;
}

// The mixer of a decimator or resampler, for offset-tuned IQ (include/adsb_hip.h, "Frequency shift").
#[link(name = "adsb_hip")]
unsafe extern "C" {
    pub fn adsb_mix_set_decim(d: *mut AdsbDecim, cs_pairs: *const i16, period: u32) -> c_int;
    pub fn adsb_mix_set_resamp(r: *mut AdsbResamp, cs_pairs: *const i16, period: u32) -> c_int;
    pub fn adsb_mix_get_decim(d: *const AdsbDecim) -> u32;
    pub fn adsb_mix_get_resamp(r: *const AdsbResamp) -> u32;
    pub fn adsb_mix_table(k: u32, period: u32, cs_pairs: *mut i16, cap: usize) -> c_int;
    pub fn adsb_mix_for_shift(up: u32, down: u32, shift_hz: i32, k: *mut u32, period: *mut u32) -> c_int;
}

// The CF32 scale of a decimator or resampler (include/adsb_hip.h, "Sample formats"); compared with the header by
// tests/test_formats_in_cpu.py.
#[link(name = "adsb_hip")]
unsafe extern "C" {
    pub fn adsb_fmt_set_scale_decim(d: *mut AdsbDecim, scale: f32) -> c_int;
    pub fn adsb_fmt_set_scale_resamp(r: *mut AdsbResamp, scale: f32) -> c_int;
    pub fn adsb_fmt_get_scale_decim(d: *const AdsbDecim) -> f32;
    pub fn adsb_fmt_get_scale_resamp(r: *const AdsbResamp) -> f32;
}

// The input statistics of a decimator, a resampler or a bank (include/adsb_hip.h, "Input statistics"; the header marks the
// calls ADSB_MUST_CHECK or `extern`); compared with the header by tests/test_instat_cpu.py.
#[link(name = "adsb_hip")]
unsafe extern "C" {
    pub fn adsb_instat_set_decim(d: *mut AdsbDecim, enabled: c_int) -> c_int;
    pub fn adsb_instat_set_resamp(r: *mut AdsbResamp, enabled: c_int) -> c_int;
    pub fn adsb_instat_set_bank(b: *mut AdsbBank, enabled: c_int) -> c_int;
    pub fn adsb_instat_get_decim(d: *const AdsbDecim) -> c_int;
    pub fn adsb_instat_get_resamp(r: *const AdsbResamp) -> c_int;
    pub fn adsb_instat_get_bank(b: *const AdsbBank) -> c_int;
    pub fn adsb_instat_fetch_decim(d: *mut AdsbDecim, out: *mut AdsbInputStats) -> c_int;
    pub fn adsb_instat_fetch_resamp(r: *mut AdsbResamp, out: *mut AdsbInputStats) -> c_int;
    pub fn adsb_instat_fetch_bank(b: *mut AdsbBank, first_stream: u32, n_streams: u32, out: *mut AdsbInputStats) -> c_int;
    pub fn adsb_input_bin(v: i16) -> c_int;
    pub fn adsb_input_summary(s: *const AdsbInputStats, n: usize, out: *mut AdsbInputSummary) -> c_int;
    pub fn adsb_instat_selftest_geometry(format: c_int, tile_samples: *mut u32, max_groups_per_run: *mut u32) -> c_int;
    pub fn adsb_instat_selftest_launches_decim(d: *const AdsbDecim) -> u64;
    pub fn adsb_instat_selftest_launches_resamp(r: *const AdsbResamp) -> u64;
    pub fn adsb_instat_selftest_launches_bank(b: *const AdsbBank) -> u64;
}
