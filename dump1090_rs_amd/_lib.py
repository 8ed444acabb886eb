"""ctypes binding of libadsb_hip.so (include/adsb_hip.h).  No fallback: if the HIP
library is missing this raises, it never routes anywhere else."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "libadsb_hip.so"

ADSB_OK = 0
ADSB_ERR_INVALID = -1
ADSB_ERR_NO_DEVICE = -2
ADSB_ERR_HIP = -3
ADSB_ERR_TOO_LONG = -4
ADSB_ERR_CAPACITY = -5
ADSB_ERR_NOMEM = -6
ADSB_ERR_BUSY = -7
ADSB_ERR_POISONED = -8
ADSB_WAIT_AUTO, ADSB_WAIT_SPIN, ADSB_WAIT_BLOCK = 0, 1, 2
ADSB_FIX_NONE, ADSB_FIX_1BIT = 0, 1
ADSB_SCORE_FIXED_1BIT = 1200
ADSB_FIX_2BIT = 3
ADSB_SCORE_FIXED_2BIT = 1100
ADSB_FAULT_PHASE1, ADSB_FAULT_PHASE2, ADSB_FAULT_HANG, ADSB_FAULT_RECORDS = 1, 2, 3, 4
ADSB_MAX_RECEIVERS = 16384
ADSB_DECIM_CS16, ADSB_DECIM_8BIT = 0, 1
ADSB_DECIM_CF32, ADSB_DECIM_REAL16 = 2, 3


class AdsbMsg(C.Structure):
    """adsb_msg (include/adsb_hip.h) == ModeSMessage + provenance."""
    _fields_ = [
        ("msg", C.c_uint8 * 14),
        ("len", C.c_uint8),
        ("try_phase", C.c_uint8),
        ("score", C.c_int32),
        ("j", C.c_uint32),
        ("chunk", C.c_uint64),
        ("signal_level", C.c_double),
    ]


class AdsbStats(C.Structure):
    _fields_ = [
        ("n_samples", C.c_uint64),
        ("n_chunks", C.c_uint64),
        ("n_candidates", C.c_uint64),
        ("n_ap_entries", C.c_uint64),
        ("n_records", C.c_uint64),
        ("n_messages", C.c_uint64),
        ("ms_scan", C.c_float),
        ("ms_match", C.c_float),
        ("ms_records", C.c_float),
        ("ms_total_device", C.c_float),
        ("retries", C.c_uint32),
        ("ms_scan_exclusive", C.c_float),
    ]


class AdsbTrial(C.Structure):
    """adsb_trial (include/adsb_hip.h): one raw trial message, before scoring."""
    _fields_ = [
        ("power", C.c_uint64),
        ("chunk", C.c_uint32),
        ("j_tp", C.c_uint32),
        ("msg", C.c_uint8 * 14),
        ("pad", C.c_uint16),
    ]


class AdsbMultiStats(C.Structure):
    """adsb_multi_stats (include/adsb_hip.h): the capture an adsb_multi collected last."""
    _fields_ = [
        ("n_samples", C.c_uint64),
        ("n_chunks", C.c_uint64),
        ("n_candidates", C.c_uint64),
        ("n_ap_entries", C.c_uint64),
        ("n_records", C.c_uint64),
        ("n_messages", C.c_uint64),
        ("n_addrs_exchanged", C.c_uint64),
        ("n_devices", C.c_uint32),
        ("retries", C.c_uint32),
        ("ms_wall", C.c_float),
        ("ms_phase1_max", C.c_float),
        ("ms_phase2_max", C.c_float),
        ("ms_phase1_span", C.c_float),
        ("ms_phase2_span", C.c_float),
        ("ms_exchange", C.c_float),
        ("ms_replay", C.c_float),
        ("reserved", C.c_float),
    ]


class AdsbSignalStats(C.Structure):
    """adsb_signal_stats (include/adsb_hip.h, "Signal statistics"): one buffer's integer record.  272 bytes."""
    _fields_ = [
        ("chunk", C.c_uint64),
        ("sum_power", C.c_uint64),
        ("n_samples", C.c_uint32),
        ("peak", C.c_uint32),
        ("n_strong", C.c_uint32),
        ("n_clipped", C.c_uint32),
        ("hist", C.c_uint32 * 60),
    ]


class AdsbSignalSummary(C.Structure):
    """adsb_signal_summary_t: what adsb_signal_summary makes of any number of records."""
    _fields_ = [
        ("n_buffers", C.c_uint64),
        ("n_samples", C.c_uint64),
        ("mean_power_dbfs", C.c_double),
        ("peak_dbfs", C.c_double),
        ("median_dbfs", C.c_double),
        ("clipped_fraction", C.c_double),
        ("strong_fraction", C.c_double),
    ]


ADSB_INPUT_BINS = 17


class AdsbInputStats(C.Structure):
    """adsb_input_stats (include/adsb_hip.h, "Input statistics"): the integer record of a set of raw input samples of a
    decimator, a resampler or one stream of a bank.  208 bytes."""
    _fields_ = [
        ("n_samples", C.c_uint64),
        ("sum_re", C.c_int64),
        ("sum_im", C.c_int64),
        ("sum_re2", C.c_uint64),
        ("sum_im2", C.c_uint64),
        ("sum_re_im", C.c_int64),
        ("n_clipped", C.c_uint64),
        ("n_nan", C.c_uint64),
        ("hist", C.c_uint64 * ADSB_INPUT_BINS),
        ("peak", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class AdsbInputSummary(C.Structure):
    """adsb_input_summary_t: what adsb_input_summary makes of any number of records."""
    _fields_ = [
        ("n_records", C.c_uint64),
        ("n_samples", C.c_uint64),
        ("mean_power_dbfs", C.c_double),
        ("peak_dbfs", C.c_double),
        ("dc_re", C.c_double),
        ("dc_im", C.c_double),
        ("clipped_fraction", C.c_double),
        ("nan_fraction", C.c_double),
        ("iq_gain_db", C.c_double),
        ("bits_used", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class AdsbError(RuntimeError):
    def __init__(self, status: int, what: str, detail: str = ""):
        self.status = status
        super().__init__(f"{what}: {detail}" if detail else what)


_lib = None


def lib() -> C.CDLL:
    """Load libadsb_hip.so (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m dump1090_rs_amd.build` "
            "(there is no CPU fallback for the demod_2400 path)")
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7.
    # If this library pulled in /opt/rocm's copy first, a later `import torch` would find
    # "No HIP GPUs".  Loading torch first (when it is installed) makes both share
    # torch's runtime; without torch (a C/Rust host) the RUNPATH copy is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(str(LIB_PATH))
    vp, sz = C.c_void_p, C.c_size_t
    L.adsb_create.argtypes = [C.POINTER(vp), C.c_int, sz]
    L.adsb_destroy.argtypes = [vp]
    L.adsb_destroy.restype = None
    L.adsb_set_stream.argtypes = [vp, vp]
    L.adsb_set_profiling.argtypes = [vp, C.c_int]
    L.adsb_icao_flush.argtypes = [vp]
    L.adsb_to_mag.argtypes = [vp, vp, sz, vp, C.POINTER(sz)]
    L.adsb_demodulate2400.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_demod_iq.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_demod_iq_device.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_submit_iq_device.argtypes = [vp, vp, sz]
    L.adsb_collect.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.adsb_pending.argtypes = [vp]
    L.adsb_max_in_flight.argtypes = [vp]
    L.adsb_max_in_flight.restype = C.c_int
    L.adsb_fetch_messages.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.adsb_ring_create.argtypes = [vp, sz]
    L.adsb_ring_acquire.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.adsb_ring_submit.argtypes = [vp, sz]
    L.adsb_set_u8_table.argtypes = [vp, vp]
    L.adsb_to_mag_u8.argtypes = [vp, vp, sz, vp, C.POINTER(sz)]
    L.adsb_demod_iq_u8.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_demod_iq_device_u8.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_submit_iq_device_u8.argtypes = [vp, vp, sz]
    L.adsb_ring_create_u8.argtypes = [vp, sz]
    L.adsb_ring_acquire_u8.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.adsb_selftest_u8_table.argtypes = [vp, vp]
    L.adsb_read_test_data.argtypes = [C.c_char_p, vp, sz, C.POINTER(sz)]
    L.adsb_get_stats.argtypes = [vp, C.POINTER(AdsbStats)]
    L.adsb_replay_records.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_set_carry_over.argtypes = [vp, C.c_int]
    L.adsb_set_carry_over.restype = C.c_int
    L.adsb_set_error_correction.argtypes = [vp, C.c_int]
    L.adsb_set_error_correction.restype = C.c_int
    L.adsb_get_error_correction.argtypes = [vp]
    L.adsb_get_error_correction.restype = C.c_int
    L.adsb_set_signal_stats.argtypes = [vp, C.c_int]
    L.adsb_set_signal_stats.restype = C.c_int
    L.adsb_get_signal_stats.argtypes = [vp]
    L.adsb_get_signal_stats.restype = C.c_int
    L.adsb_fetch_signal_stats.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.adsb_fetch_signal_stats.restype = C.c_int
    L.adsb_signal_bin.argtypes = [C.c_uint16]
    L.adsb_signal_bin.restype = C.c_int
    L.adsb_signal_summary.argtypes = [vp, sz, C.POINTER(AdsbSignalSummary)]
    L.adsb_signal_summary.restype = C.c_int
    L.adsb_selftest_signal_launches.argtypes = [vp]
    L.adsb_selftest_signal_launches.restype = C.c_uint64
    L.adsb_replay_records_fix.argtypes = [vp, vp, sz, C.c_int, vp, sz, C.POINTER(sz)]
    L.adsb_replay_records_fix.restype = C.c_int
    L.adsb_selftest_fix_table.argtypes = [vp]
    L.adsb_selftest_fix_table.restype = C.c_int
    L.adsb_selftest_fix_hash.argtypes = [C.POINTER(C.c_uint32), vp, sz]
    L.adsb_selftest_fix_hash.restype = C.c_int
    L.adsb_selftest_fix2_table.argtypes = [vp, vp, sz]
    L.adsb_selftest_fix2_table.restype = C.c_int
    L.adsb_selftest_fix_lookup.argtypes = [vp, vp, sz, C.c_int, vp]
    L.adsb_selftest_fix_lookup.restype = C.c_int
    L.adsb_selftest_parallel_replay_fix.argtypes = [vp, vp, sz, C.c_int, C.c_int, C.c_int, C.c_int, vp, sz, C.POINTER(sz),
                                                    C.POINTER(C.c_int)]
    L.adsb_selftest_parallel_replay_fix.restype = C.c_int
    L.adsb_format_raw.argtypes = [vp, C.c_char_p, sz]
    L.adsb_format_raw.restype = C.c_int
    L.adsb_shard_scan.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_shard_finish.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_selftest_mag_digest.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.adsb_strerror.argtypes = [C.c_int]
    L.adsb_strerror.restype = C.c_char_p
    L.adsb_last_error.argtypes = [vp]
    L.adsb_last_error.restype = C.c_char_p
    L.adsb_version.restype = C.c_char_p
    L.adsb_selftest_stage_lists.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]
    L.adsb_selftest_stage_lists.restype = C.c_int
    L.adsb_selftest_gate_stages.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz)]
    L.adsb_selftest_gate_stages.restype = C.c_int
    L.adsb_selftest_set_order_polls.argtypes = [vp, C.c_uint32]
    L.adsb_selftest_set_order_polls.restype = C.c_int
    # (hooks reached by name, not declared in include/adsb_hip.h: k_scan_sparse on / off for a context, and its launches)
    L.adsb_selftest_set_sparse_scan.argtypes = [vp, C.c_int]
    L.adsb_selftest_set_sparse_scan.restype = C.c_int
    L.adsb_selftest_sparse_scans.argtypes = [vp]
    L.adsb_selftest_sparse_scans.restype = C.c_uint64
    L.adsb_selftest_crc_table.argtypes = [vp]
    L.adsb_selftest_crc_table.restype = C.c_int
    L.adsb_selftest_learned_union.argtypes = [vp, sz, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_selftest_learned_union.restype = C.c_int
    ip = C.POINTER(C.c_int)
    L.adsb_multi_create.argtypes = [C.POINTER(vp), ip, C.c_int, sz]
    L.adsb_multi_destroy.argtypes = [vp]
    L.adsb_multi_destroy.restype = None
    L.adsb_multi_device_count.argtypes = [vp]
    L.adsb_multi_max_in_flight.argtypes = [vp]
    L.adsb_multi_shard_range.argtypes = [sz, C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]
    L.adsb_multi_icao_flush.argtypes = [vp]
    L.adsb_multi_demod_iq.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_multi_demod_iq_device.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), vp, sz, C.POINTER(sz)]
    L.adsb_multi_submit_iq_device.argtypes = [vp, C.POINTER(vp), C.POINTER(sz)]
    L.adsb_multi_submit_iq.argtypes = [vp, vp, sz]
    L.adsb_multi_host_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.adsb_multi_host_free.argtypes = [vp, vp]
    L.adsb_multi_collect.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.adsb_multi_selftest_tune.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32]
    L.adsb_multi_selftest_tune.restype = C.c_int
    L.adsb_multi_selftest_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.adsb_multi_selftest_counters.restype = C.c_int
    L.adsb_multi_pending.argtypes = [vp]
    L.adsb_multi_set_wait.argtypes = [vp, C.c_int]
    L.adsb_multi_get_wait.argtypes = [vp]
    L.adsb_multi_set_timeout_ms.argtypes = [vp, C.c_uint32]
    L.adsb_multi_set_error_correction.argtypes = [vp, C.c_int]
    L.adsb_multi_set_error_correction.restype = C.c_int
    L.adsb_multi_selftest_fail.argtypes = [vp, C.c_uint32, C.c_int, C.c_int]
    L.adsb_multi_fetch_messages.argtypes = [vp, vp, sz, C.POINTER(sz)]
    L.adsb_multi_get_stats.argtypes = [vp, C.POINTER(AdsbMultiStats)]
    L.adsb_multi_filter_table.argtypes = [vp, vp]
    L.adsb_multi_last_error.argtypes = [vp]
    L.adsb_multi_last_error.restype = C.c_char_p
    for name in ("adsb_multi_create", "adsb_multi_device_count", "adsb_multi_max_in_flight", "adsb_multi_shard_range",
                 "adsb_multi_icao_flush", "adsb_multi_demod_iq", "adsb_multi_demod_iq_device", "adsb_multi_submit_iq_device",
                 "adsb_multi_submit_iq", "adsb_multi_host_alloc", "adsb_multi_host_free",
                 "adsb_multi_collect", "adsb_multi_pending", "adsb_multi_fetch_messages", "adsb_multi_get_stats",
                 "adsb_multi_filter_table", "adsb_multi_set_wait", "adsb_multi_get_wait", "adsb_multi_set_timeout_ms",
                 "adsb_multi_selftest_fail"):
        getattr(L, name).restype = C.c_int
    # many receivers, one pass (include/adsb_hip.h)
    u32 = C.c_uint32
    L.adsb_set_receivers.argtypes = [vp, u32]
    L.adsb_get_receivers.argtypes = [vp]
    L.adsb_icao_flush_receiver.argtypes = [vp, u32]
    L.adsb_receiver_filter_table.argtypes = [vp, u32, vp]
    for name in ("adsb_demod_iq_rx", "adsb_demod_iq_device_rx", "adsb_demod_iq_rx_u8", "adsb_demod_iq_device_rx_u8"):
        getattr(L, name).argtypes = [vp, vp, sz, vp, vp, sz, C.POINTER(sz)]
    L.adsb_submit_iq_device_rx.argtypes = [vp, vp, sz, vp]
    L.adsb_submit_iq_device_rx_u8.argtypes = [vp, vp, sz, vp]
    L.adsb_ring_submit_rx.argtypes = [vp, sz, vp]
    L.adsb_replay_records_rx.argtypes = [vp, u32, vp, sz, vp, sz, C.c_int, C.c_int, vp, sz, C.POINTER(sz)]
    L.adsb_selftest_rx_tune.argtypes = [vp, u32]
    L.adsb_selftest_rx_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.adsb_set_receiver_scoring.argtypes = [vp, C.c_int]
    L.adsb_get_receiver_scoring.argtypes = [vp]
    L.adsb_selftest_rx_score_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.adsb_selftest_rx_score_tune.argtypes = [vp, u32, u32]
    L.adsb_selftest_rx_set_lookup.argtypes = [vp, vp, sz, vp, sz, vp]
    L.adsb_rx_set_home.argtypes = [C.c_uint64, u32]
    L.adsb_set_receiver_carry.argtypes = [vp, C.c_int]
    L.adsb_get_receiver_carry.argtypes = [vp]
    L.adsb_receiver_carry_reset.argtypes = [vp, u32]
    L.adsb_selftest_rx_seam_tune.argtypes = [vp, u32]
    L.adsb_selftest_rx_seam_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.adsb_set_receiver_carry_scoring.argtypes = [vp, C.c_int]
    L.adsb_get_receiver_carry_scoring.argtypes = [vp]
    L.adsb_selftest_rx_seam_score_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.adsb_selftest_reservations.argtypes = [vp]
    L.adsb_selftest_reservations.restype = C.c_uint64
    for name in ("adsb_set_receiver_carry", "adsb_get_receiver_carry", "adsb_receiver_carry_reset", "adsb_selftest_rx_seam_tune",
                 "adsb_selftest_rx_seam_counters", "adsb_set_receiver_carry_scoring", "adsb_get_receiver_carry_scoring",
                 "adsb_selftest_rx_seam_score_counters"):
        getattr(L, name).restype = C.c_int
    L.adsb_rx_set_home.restype = u32
    for name in ("adsb_set_receiver_scoring", "adsb_get_receiver_scoring", "adsb_selftest_rx_score_counters",
                 "adsb_selftest_rx_score_tune", "adsb_selftest_rx_set_lookup"):
        getattr(L, name).restype = C.c_int
    for name in ("adsb_set_receivers", "adsb_get_receivers", "adsb_icao_flush_receiver", "adsb_receiver_filter_table",
                 "adsb_demod_iq_rx", "adsb_demod_iq_device_rx", "adsb_demod_iq_rx_u8", "adsb_demod_iq_device_rx_u8",
                 "adsb_submit_iq_device_rx", "adsb_submit_iq_device_rx_u8", "adsb_ring_submit_rx", "adsb_replay_records_rx",
                 "adsb_selftest_rx_tune", "adsb_selftest_rx_counters"):
        getattr(L, name).restype = C.c_int
    # decimation (include/adsb_hip.h)
    i16p, u32p = C.POINTER(C.c_int16), C.POINTER(u32)
    L.adsb_decim_create.argtypes = [vp, u32, vp, u32, u32, C.POINTER(vp)]
    L.adsb_decim_destroy.argtypes = [vp]
    L.adsb_decim_destroy.restype = None
    L.adsb_decim_reset.argtypes = [vp]
    L.adsb_decim_out_count.argtypes = [vp, sz, C.POINTER(sz)]
    L.adsb_decim_run_device.argtypes = [vp, C.c_int, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_decim_demod_iq.argtypes = [vp, C.c_int, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_decim_default_taps.argtypes = [u32, i16p, sz, u32p, u32p]
    L.adsb_decim_selftest_tile.argtypes = []
    L.adsb_decim_selftest_tile.restype = u32
    for name in ("adsb_decim_create", "adsb_decim_reset", "adsb_decim_out_count", "adsb_decim_run_device",
                 "adsb_decim_demod_iq", "adsb_decim_default_taps"):
        getattr(L, name).restype = C.c_int
    # resampling (include/adsb_hip.h)
    u64, u64p = C.c_uint64, C.POINTER(C.c_uint64)
    L.adsb_resamp_create.argtypes = [vp, u32, u32, vp, u32, u32, C.POINTER(vp)]
    L.adsb_resamp_destroy.argtypes = [vp]
    L.adsb_resamp_destroy.restype = None
    L.adsb_resamp_reset.argtypes = [vp]
    L.adsb_resamp_out_count.argtypes = [vp, sz, C.POINTER(sz)]
    L.adsb_resamp_run_device.argtypes = [vp, C.c_int, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_resamp_demod_iq.argtypes = [vp, C.c_int, vp, sz, vp, sz, C.POINTER(sz)]
    L.adsb_resamp_default_taps.argtypes = [u32, u32, i16p, sz, u32p, u32p]
    L.adsb_resamp_ratio_for_rate.argtypes = [u32, u32p, u32p]
    L.adsb_resamp_plan.argtypes = [u32, u32, u64, u64, u64p, u64p]
    L.adsb_resamp_selftest_tile.argtypes = [u32, u32]
    L.adsb_resamp_selftest_tile.restype = u32
    for name in ("adsb_resamp_create", "adsb_resamp_reset", "adsb_resamp_out_count", "adsb_resamp_run_device",
                 "adsb_resamp_demod_iq", "adsb_resamp_default_taps", "adsb_resamp_ratio_for_rate", "adsb_resamp_plan"):
        getattr(L, name).restype = C.c_int
    # frequency shift (include/adsb_hip.h)
    L.adsb_mix_set_decim.argtypes = [vp, vp, u32]
    L.adsb_mix_set_resamp.argtypes = [vp, vp, u32]
    L.adsb_mix_get_decim.argtypes = [vp]
    L.adsb_mix_get_resamp.argtypes = [vp]
    L.adsb_mix_table.argtypes = [u32, u32, i16p, sz]
    L.adsb_mix_for_shift.argtypes = [u32, u32, C.c_int32, u32p, u32p]
    for name in ("adsb_mix_get_decim", "adsb_mix_get_resamp"):
        getattr(L, name).restype = u32
    for name in ("adsb_mix_set_decim", "adsb_mix_set_resamp", "adsb_mix_table", "adsb_mix_for_shift"):
        getattr(L, name).restype = C.c_int
    # sample formats (include/adsb_hip.h)
    for name in ("adsb_fmt_set_scale_decim", "adsb_fmt_set_scale_resamp"):
        getattr(L, name).argtypes = [vp, C.c_float]
        getattr(L, name).restype = C.c_int
    for name in ("adsb_fmt_get_scale_decim", "adsb_fmt_get_scale_resamp"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = C.c_float
    # resampler banks (include/adsb_hip.h)
    szp = C.POINTER(sz)
    L.adsb_bank_create.argtypes = [vp, u32, u32, u32, vp, u32, u32, C.POINTER(vp)]
    L.adsb_bank_destroy.argtypes = [vp]
    L.adsb_bank_destroy.restype = None
    L.adsb_bank_streams.argtypes = [vp]
    L.adsb_bank_reset.argtypes = [vp, u32]
    L.adsb_bank_consumed.argtypes = [vp, u32, u64p]
    L.adsb_bank_out_count.argtypes = [vp, u32, sz, szp]
    L.adsb_bank_inputs_for.argtypes = [vp, u32, sz, szp, szp]
    L.adsb_bank_run_device.argtypes = [vp, C.c_int, u32, vp, vp, vp, vp, vp, vp]
    L.adsb_bank_set_mixer.argtypes = [vp, vp, u32]
    L.adsb_bank_get_mixer.argtypes = [vp]
    L.adsb_bank_set_scale.argtypes = [vp, C.c_float]
    L.adsb_bank_get_scale.argtypes = [vp]
    L.adsb_bank_get_scale.restype = C.c_float
    L.adsb_bank_selftest_depth.argtypes = []
    for name in ("adsb_bank_streams", "adsb_bank_get_mixer", "adsb_bank_selftest_depth"):
        getattr(L, name).restype = u32
    for name in ("adsb_bank_create", "adsb_bank_reset", "adsb_bank_consumed", "adsb_bank_out_count", "adsb_bank_inputs_for",
                 "adsb_bank_run_device", "adsb_bank_set_mixer", "adsb_bank_set_scale"):
        getattr(L, name).restype = C.c_int
    # input statistics (include/adsb_hip.h)
    stp = C.POINTER(AdsbInputStats)
    for kind in ("decim", "resamp", "bank"):
        getattr(L, f"adsb_instat_set_{kind}").argtypes = [vp, C.c_int]
        getattr(L, f"adsb_instat_get_{kind}").argtypes = [vp]
        getattr(L, f"adsb_instat_fetch_{kind}").argtypes = [vp, u32, u32, stp] if kind == "bank" else [vp, stp]
        getattr(L, f"adsb_instat_selftest_launches_{kind}").argtypes = [vp]
        getattr(L, f"adsb_instat_selftest_launches_{kind}").restype = u64
        for call in ("set", "get", "fetch"):
            getattr(L, f"adsb_instat_{call}_{kind}").restype = C.c_int
    L.adsb_input_bin.argtypes = [C.c_int16]
    L.adsb_input_bin.restype = C.c_int
    L.adsb_input_summary.argtypes = [stp, sz, C.POINTER(AdsbInputSummary)]
    L.adsb_input_summary.restype = C.c_int
    L.adsb_instat_selftest_geometry.argtypes = [C.c_int, u32p, u32p]
    L.adsb_instat_selftest_geometry.restype = C.c_int
    L.adsb_host_replays.argtypes = [vp]
    L.adsb_host_replays.restype = C.c_uint64
    L.adsb_host_register.argtypes = [vp, C.c_void_p, C.c_size_t]
    L.adsb_host_register.restype = C.c_int
    L.adsb_host_unregister.argtypes = [vp, C.c_void_p]
    L.adsb_host_unregister.restype = C.c_int
    L.adsb_host_rematches.argtypes = [vp]
    L.adsb_host_rematches.restype = C.c_uint64
    L.adsb_host_sorts.argtypes = [vp]
    L.adsb_host_sorts.restype = C.c_uint64
    for name in ("adsb_create", "adsb_set_stream", "adsb_set_profiling", "adsb_icao_flush",
                 "adsb_to_mag", "adsb_demodulate2400", "adsb_demod_iq", "adsb_demod_iq_device",
                 "adsb_read_test_data", "adsb_get_stats", "adsb_replay_records",
                 "adsb_selftest_mag_digest", "adsb_submit_iq_device", "adsb_collect", "adsb_pending",
                 "adsb_fetch_messages",
                 "adsb_ring_create", "adsb_ring_acquire", "adsb_ring_submit", "adsb_shard_scan",
                 "adsb_shard_finish"):
        getattr(L, name).restype = C.c_int
    _lib = L
    return L
